"""The cases the HDR stream's tests share: frame sizes, stream configurations and the injected layer sets."""
from test_gpu_grade import layer_sets  # noqa: F401  (zeros, the toe ramp, noise, 1e4, 65504 and the non-finite ones)

# one thread; 2-byte chroma rows; more than one 32 x 8 thread block each way, with partial blocks
SIZES = [(2, 2), (6, 4), (66, 18), (130, 34)]
EXPOSURES = (-2.0, 0.0, 1.5)
WHITES = (100.0, 203.0, 1000.0)
CONFIGS = [dict(transfer="pq", exposure=e, white_nits=w) for e in EXPOSURES for w in WHITES] + \
          [dict(transfer="hlg", exposure=e, white_nits=203.0) for e in EXPOSURES]
