"""The grid of (net, batch, frames) over which the sizes of the training work buffers are pinned, and the seven size queries
in the order of the fixture's columns.  Shared by tools/dump_train_work_sizes.py, which records the fixture
tests/golden/train_work_sizes.json, and tests/test_train_work_host.py, which compares the library against it.

The shapes put rows on both sides of every predicate that changes a layout: Tp >= 256 (REF6 at 2 frames against 3, tiny at 3
frames against 14), the 2 GiB reach test of swn_drop_g16 (REF6 at (2, 31) against (8, 1100)), that of swn_bl6_bwd_supported
((16, 1100) for bl6_laplace(1, 0)), seg == 1 against seg > 1, Laplace against softmax, and the two refusals."""
import ctypes
from dataclasses import asdict

from shallow_wavenet_amd import config as C

NETS = (
    ("tiny_laplace_1_0", C.tiny("laplace", 1, 0)),
    ("tiny_laplace_2_4", C.tiny("laplace", 2, 4)),
    ("tiny_softmax", C.tiny("softmax")),
    ("bl6_laplace_1_0", C.bl6_laplace(1, 0)),
    ("bl6_laplace_5_4", C.bl6_laplace(5, 4)),
    ("bl6_softmax", C.bl6_softmax()),
    ("ref6_laplace_1_4", C.ref6_laplace(1, 4)),
    ("ref6_laplace_5_4", C.ref6_laplace(5, 4)),
    ("ref6_softmax", C.ref6_softmax()),
)
SHAPES = ((1, 1), (1, 2), (2, 3), (3, 14), (2, 31), (8, 1100), (16, 1100), (64, 150), (0, 4), (2, 0))
REFUSALS = ((0, 4), (2, 0))
QUERIES = (
    "swn_forward_work_floats",
    "swn_forward_drop_work_floats",
    "swn_forward_bf16_work_bytes",
    "swn_forward_bf16_keep_floats",
    "swn_backward_work_floats",
    "swn_backward_bf16_work_floats",
    "swn_backward_drop_work_floats",
)


def query_sizes(lib, cfg, batch, frames):
    from shallow_wavenet_amd import _lib
    d = _lib.desc_from_cfg(cfg)
    return [int(getattr(lib, q)(ctypes.byref(d), batch, frames)) for q in QUERIES]


def rows(lib):
    return [dict(net=name, cfg=asdict(cfg), batch=b, frames=f, sizes=query_sizes(lib, cfg, b, f))
            for name, cfg in NETS for b, f in SHAPES]
