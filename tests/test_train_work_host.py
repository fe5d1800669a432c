"""Sizes of the training work buffers (host arithmetic of csrc/swn_train_internal.hpp; no GPU).

tests/golden/train_work_sizes.json holds what the seven size queries answered at the commit before the layouts moved into
one header, over the grid of tests/train_work_grid.py (tools/dump_train_work_sizes.py recorded it from a library built from
that commit).  A work buffer's layout is a data format between a size query and the calls that carve the buffer: every
query must keep answering byte for byte what it answered then.  A row may change only together with a fix of a call that
wrote past its query's size, and then tools/dump_train_work_sizes.py records it again.

(16, 1100) was added to the grid to take bl6_laplace(1, 0) past the reach test of swn_bl6_bwd_supported: it does - one
utterance set's hidden states, 16 * 7 * 64 * 120 999 * 4 bytes = 3.5 GB, exceed the kernels' 32-bit offsets, and
swn_backward_bf16_work_floats answers 0 there while (8, 1100) (1.7 GB) is served; test_bl6_reach_row asserts both."""
import json
import os
from dataclasses import asdict

import pytest

import train_work_grid as G
from conftest import GOLDEN_DIR
from shallow_wavenet_amd import _lib
from shallow_wavenet_amd.config import NetConfig


def _fixture():
    with open(os.path.join(GOLDEN_DIR, "train_work_sizes.json")) as f:
        return json.load(f)


FIX = _fixture()
ROWS = {(r["net"], r["batch"], r["frames"]): r for r in FIX["rows"]}
Q = {q: i for i, q in enumerate(G.QUERIES)}


def test_fixture_covers_the_grid():
    assert FIX["queries"] == list(G.QUERIES)
    assert len(G.NETS) == 9 and len(G.SHAPES) == 10 and len(FIX["rows"]) == 90
    for name, cfg in G.NETS:
        for b, f in G.SHAPES:
            assert NetConfig(**ROWS[(name, b, f)]["cfg"]) == cfg, (name, b, f)


@pytest.mark.parametrize("name,cfg", G.NETS, ids=[n for n, _ in G.NETS])
def test_sizes_match_the_recorded_ones(name, cfg):
    lib = _lib.lib()
    for b, f in G.SHAPES:
        got = G.query_sizes(lib, cfg, b, f)
        want = ROWS[(name, b, f)]["sizes"]
        assert got == want, (name, b, f, dict(zip(G.QUERIES, zip(got, want))))


def test_recorded_rows_are_the_classes_they_stand_for():
    """the fixture itself: refusals answer 0 everywhere, every other row is non-zero wherever its class applies"""
    for (name, b, f), r in ROWS.items():
        s = r["sizes"]
        if (b, f) in G.REFUSALS:
            assert s == [0] * 7, (name, b, f)
            continue
        for q in ("swn_forward_work_floats", "swn_forward_drop_work_floats", "swn_backward_work_floats",
                  "swn_backward_drop_work_floats"):
            assert s[Q[q]] > 0, (name, b, f, q)
        assert (s[Q["swn_forward_bf16_work_bytes"]] == 0) == name.startswith("tiny"), (name, b, f)
        assert (s[Q["swn_forward_bf16_keep_floats"]] > 0) == (name == "bl6_softmax" or name.startswith("ref6")), (name, b, f)
        if name != "bl6_laplace_1_0":
            assert s[Q["swn_backward_bf16_work_floats"]] == 0, (name, b, f)


def test_bl6_reach_row():
    q = Q["swn_backward_bf16_work_floats"]
    assert ROWS[("bl6_laplace_1_0", 8, 1100)]["sizes"][q] > 0
    assert ROWS[("bl6_laplace_1_0", 16, 1100)]["sizes"][q] == 0
    for b, f in G.SHAPES:
        if (b, f) not in G.REFUSALS and (b, f) != (16, 1100):
            assert ROWS[("bl6_laplace_1_0", b, f)]["sizes"][q] > 0, (b, f)
