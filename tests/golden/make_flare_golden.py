"""Generates tests/golden/flare_cases.npz: the reference's own _apply_lens_flare (render.py:3925-4028) on the GOLDEN subset of
tests/flare_cases.py -- every disk plane kind on one landscape, one portrait and one tiny frame, and the threshold trio.

    python tests/golden/make_flare_golden.py <directory of the reference's render.py>

Runs where the reference is checked out, never on a device.  The reference imports taichi / imageio at module level and
_apply_lens_flare touches neither, so empty placeholder modules are registered first, as make_golden.py does.  Arrays go in
as the reference holds them, (W, H, 3).  Only outputs are stored, keyed by case name, as (H, W, 3); the inputs are rebuilt
from the table.  tests/test_flare_ref.py holds oracle/flare_np.py to every one of them bit for bit."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import flare_cases as FC  # noqa: E402


def import_reference(ref_dir):
    for name in ("taichi", "imageio", "imageio.v3"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["imageio"].v3 = sys.modules["imageio.v3"]
    sys.path.insert(0, ref_dir)
    import render as ref  # noqa
    return ref


def generate(ref):
    out = {}
    for case in FC.GOLDEN:
        final, disk = (np.ascontiguousarray(a.transpose(1, 0, 2)) for a in FC.inputs(case))
        got = ref.TaichiRenderer._apply_lens_flare(None, final.copy(), disk.copy())
        assert got.dtype == np.float32 and got.shape == final.shape
        out[case.name] = np.ascontiguousarray(got.transpose(1, 0, 2))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = generate(import_reference(sys.argv[1]))
    path = os.path.join(HERE, "flare_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
