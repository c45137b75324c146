"""Worker of tests/test_gpu_grade.py: one rank of the one-process-per-tile row-block path, under a grade and without.
usage: python tests/grade_tile_worker.py <dir> <rank> <world> <shm name>"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    d, rank, world, shm = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    from bhr_amd import HipRenderer, _lib, multigpu, scenes
    s = scenes.SCENES["default"]
    W, H = 640, 360                                        # R = 12: tiles of 360 / world rows are thicker than the halo
    cuts = [round(H * k / world / 8) * 8 for k in range(world)] + [H]
    r = HipRenderer(W, H, scenes.analytic_skybox(), scenes.noisy_disk(), rows=(cuts[rank], cuts[rank + 1]), frame_slots=1, **s["kw"])
    link = multigpu.TileLink(r, rank, world, multigpu.file_exchange(d, rank, world), shm, gather="peer")
    r.set_grade("aces", transfer="srgb")
    try:
        link.render(s["cam_pos"], s["fov"])
    except ValueError as e:                                # BHR_ERR_INVALID at the gate: nothing launched, the link intact
        assert "grade" in str(e), e
    else:
        raise SystemExit("bhr_tile_render rendered under a grade")
    handles = _lib.TileHandles()
    assert _lib.load().bhr_tile_export(r._ctx, 0, C.byref(handles)) == _lib.BHR_ERR_INVALID
    r.set_grade(None)
    link.render(s["cam_pos"], s["fov"])
    if rank == 0:
        np.save(os.path.join(d, "frame.npy"), link.read_gathered())
    link.close()
    r.close()


if __name__ == "__main__":
    main()
