"""Motion-JPEG in MP4 (mp4.write_jpeg_mp4) over frames made by the restatement, and the CLI / driver options.  No GPU."""
import io
import os

import numpy as np
import pytest

import jpeg_ref


def _frames(tmp_path, n=5, w=48, h=32):
    paths, arrays = [], []
    y, x = np.mgrid[0:h, 0:w]
    for k in range(n):
        img = np.stack([(x * 5 + 20 * k) % 256, (y * 7) % 256, (x + y + 9 * k) % 256], axis=-1).astype(np.uint8)
        p = tmp_path / f"frame_{k:04d}.jpg"
        p.write_bytes(jpeg_ref.encode(img, 50 + 10 * k, jpeg_ref.restart_interval(w)))
        paths.append(str(p))
        arrays.append(img)
    return paths, arrays


def test_write_jpeg_mp4_samples_are_the_frame_files(tmp_path):
    from PIL import Image
    from bhr_amd import mp4
    paths, arrays = _frames(tmp_path)
    assert mp4.jpeg_size(paths[0]) == (48, 32)
    out = str(tmp_path / "v.mp4")
    total = mp4.write_jpeg_mp4(paths, 24, out, 48, 32)
    assert total == os.path.getsize(out) and not os.path.exists(out + ".part")
    info = mp4.read_samples(out)
    assert info["codec"] == "mp4v" and info["object_type"] == 0x6C == mp4.JPEG_OBJECT_TYPE
    assert (info["width"], info["height"], info["timescale"], info["duration"]) == (48, 32, 24, len(paths))
    sizes = [os.path.getsize(p) for p in paths]
    assert [s for _, s in info["samples"]] == sizes
    offs = [o for o, _ in info["samples"]]
    assert offs == [offs[0] + sum(sizes[:k]) for k in range(len(sizes))] and offs[-1] + sizes[-1] == info["file_size"]
    data = open(out, "rb").read()
    for (o, s), p, img in zip(info["samples"], paths, arrays):
        sample = data[o:o + s]
        assert sample == open(p, "rb").read()
        dec = np.asarray(Image.open(io.BytesIO(sample)).convert("RGB"))
        assert dec.shape == img.shape and np.abs(dec.astype(int) - img).mean() < 40


def test_write_jpeg_mp4_refuses_other_files(tmp_path):
    from bhr_amd import mp4
    paths, _ = _frames(tmp_path, n=2)
    png = tmp_path / "x.jpg"
    png.write_bytes(mp4.PNG_MAGIC + b"\0" * 32)
    with pytest.raises(ValueError, match="not a JPEG"):
        mp4.write_jpeg_mp4(paths + [str(png)], 24, str(tmp_path / "v.mp4"), 48, 32)
    with pytest.raises(ValueError, match="not a PNG"):
        mp4.write_png_mp4(paths, 24, str(tmp_path / "w.mp4"), 48, 32)
    with pytest.raises(ValueError, match="not a JPEG"):
        mp4.jpeg_size(str(png))
    with pytest.raises(ValueError, match="no frames"):
        mp4.write_jpeg_mp4([], 24, str(tmp_path / "v.mp4"), 48, 32)


def test_assemble_video_muxes_jpeg_frames(tmp_path):
    from bhr_amd import drivers, mp4
    paths, _ = _frames(tmp_path, n=3)
    out = str(tmp_path / "v.mp4")
    assert drivers.assemble_video(str(tmp_path), 3, 12, out, codec="mjpeg")
    info = mp4.read_samples(out)
    assert info["object_type"] == 0x6C and len(info["samples"]) == 3 and (info["width"], info["height"]) == (48, 32)
    assert not drivers.assemble_video(str(tmp_path), 4, 12, str(tmp_path / "w.mp4"), codec="mjpeg")     # frame 3 is missing
    assert not drivers.assemble_video(str(tmp_path), 3, 12, str(tmp_path / "w.mp4"))                    # no PNG frames here
    with pytest.raises(ValueError):
        drivers.assemble_video(str(tmp_path), 3, 12, out, codec="bogus")


def test_cli_options_and_driver_validation(tmp_path):
    from bhr_amd import cli, drivers
    a = cli.parse_args([])
    assert a.video_codec == "auto" and a.video_quality == 90
    a = cli.parse_args(["--video", "--video_codec", "mjpeg", "--video_quality", "75"])
    assert a.video_codec == "mjpeg" and a.video_quality == 75
    cli.validate_args(a)
    with pytest.raises(SystemExit):
        cli.parse_args(["--video_codec", "h264"])
    for q in ("0", "101"):
        with pytest.raises(ValueError, match="video_quality"):
            cli.validate_args(cli.parse_args(["--video", "--video_codec", "mjpeg", "--video_quality", q]))
    # refused before the renderer (None here) is touched, and before anything is created on disk
    out = str(tmp_path / "sub" / "v.mp4")
    with pytest.raises(ValueError, match="video_codec"):
        drivers.render_video(None, 320, 180, 4, 24, out, 90, [6, 0, 0.5], video_codec="bogus")
    for q in (0, 101):
        with pytest.raises(ValueError, match="video_quality"):
            drivers.render_video(None, 320, 180, 4, 24, out, 90, [6, 0, 0.5], video_codec="mjpeg", video_quality=q)
    assert not os.path.exists(os.path.dirname(out))
