"""Without a device: the shapes tests/test_gpu_bloom_radii.py runs reach every weight table count of the split-f16 post-pass,
each at both ends of its width range, and every width class of the V pass's epilogue."""
import bloom_radii as B


def test_width_table_covers_every_table_count_at_both_ends():
    assert B.split_nt(B.SPLIT_W_MAX) == B.SPLIT_NT_MAX and B.split_nt(B.SPLIT_W_MAX + 1) == B.SPLIT_NT_MAX + 1
    assert sorted(B.NT_ENDS) == list(range(1, B.SPLIT_NT_MAX + 1))
    for nt, (lo, hi) in B.NT_ENDS.items():
        assert B.split_nt(lo) == nt and B.split_nt(hi) == nt, (nt, lo, hi)
        assert lo == 1 or B.split_nt(lo - 1) == nt - 1, (nt, lo)          # the ends are the range's ends
        assert B.split_nt(hi + 1) == nt + 1, (nt, hi)
    assert B.radius(49) == 0 and B.radius(50) == 1 and B.radius(8849) == 176
    widths = {w for w, _ in B.shapes()}
    assert widths == set(B.WIDTHS) and max(widths) == B.SPLIT_W_MAX
    assert {B.split_nt(w) for w in widths} == set(range(1, B.SPLIT_NT_MAX + 1))
    assert {2560, 5120} <= widths
    assert any(w % 4 for w in widths)
    assert any(w % 4 == 0 and w % 32 for w in widths) and any(w % 32 == 0 for w in widths)


def test_heights_cover_the_edges_of_the_row_tiling():
    sh = B.shapes()
    heights = {h for _, h in sh}
    assert {1, 7, 31, 33} <= heights and max(heights) <= 300
    assert any(h % 32 == 5 and h > 32 for h in heights)
    for nt in range(8, B.SPLIT_NT_MAX + 1):          # a height below the radius where the band is widest
        assert any(B.split_nt(w) == nt and h < B.radius(w) for w, h in sh), nt
    for w, h in sh:
        disk, bg = B.synthetic_layers(w, h, 0)
        assert disk.shape == bg.shape == (h, w, 3) and disk.dtype == bg.dtype == "float32"
        assert disk.min() >= 0 and disk.max() <= 1.0 and bg.min() >= 0 and bg.max() < 0.7
