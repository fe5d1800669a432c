"""CPU: the geometry table of tests/frontend_geometry.py reaches every conv path of csrc/swn_frontend.hip, by the library's own
path query (swn_frontend_conv_lds_bytes, the function swn_frontend decides by), and every frame-tile and GEMM edge the GPU file
relies on; the size queries follow the geometry; and the fp32 oracle stays within a fixed fraction of its float64 run at every
row and stage, so that the bound derived from it (max(2e-6 * max(1, scale), 4 * e32)) cannot grow loose enough to hide a wrong
tap."""
import ctypes

import pytest
import torch

import frontend_geometry as G
from oracle import cpu_ref
from shallow_wavenet_amd import _lib
from shallow_wavenet_amd.runtime import pack_state_dict
from shallow_wavenet_amd.streaming import lookahead_frames

IDS = [r.id for r in G.ROWS]


def _lds(row):
    return [G.query_lds(_lib.lib(), row.cfg, i) for i in range(row.cfg.aux_dilation_size)]


def test_query_is_exported_and_refuses_what_it_cannot_answer():
    lib = _lib.lib()
    assert hasattr(lib, "swn_frontend_conv_lds_bytes") and "swn_frontend_conv_lds_bytes" in _lib.SIGNATURES
    cfg = G.BY_ID["k3l3_a12"].cfg
    assert G.query_lds(lib, cfg, -1) == 0 and G.query_lds(lib, cfg, 3) == 0 and G.query_lds(lib, cfg, 2) == 56160
    d = _lib.desc_from_cfg(cfg)
    d.aux_kernel_size = 4
    assert lib.swn_frontend_conv_lds_bytes(ctypes.byref(d), 0) == 0
    assert lib.swn_frontend_conv_lds_bytes(None, 0) == 0


@pytest.mark.parametrize("row", G.ROWS, ids=IDS)
def test_query_follows_the_formula_at_every_layer(row):
    got = _lds(row)
    assert got == [G.expected_lds(row.cfg, i) for i in range(row.cfg.aux_dilation_size)]
    assert max(got) == row.lds
    # the library accepts the net and packs it (nothing smaller would do: hid_chn >= 4, one skip channel, K >= 2)
    d = _lib.desc_from_cfg(row.cfg)
    assert _lib.lib().swn_packed_floats(ctypes.byref(d)) > 0
    assert pack_state_dict(row.cfg, G.state_dict(row)).numel() == _lib.lib().swn_packed_floats(ctypes.byref(d))


def test_every_row_reaches_the_path_it_is_listed_for():
    lds = {r.id: _lds(r) for r in G.ROWS}
    cfg = {r.id: r.cfg for r in G.ROWS}
    # staged without the attribute; A0 = 3, A0p = 4
    assert lds["k3l1_a1"] == [456] and cfg["k3l1_a1"].A0 == 3
    # layer 2 staged below 48 KB, layer 3 above 150 KB: unstaged ks = 3 at dilation 27
    assert lds["k3l4_a9"] == [4104, 12744, 42120, 0] and max(lds["k3l4_a9"]) <= G.LDS_DEFAULT
    assert G.lds_formula(243, 27) == 161352 > G.LDS_MAX and G.layers(cfg["k3l4_a9"])[3][2] == 27
    # ... and the same dilation-27 layer STAGED (n_aux 8: 216 input rows): the widest window the LDS kernel takes, 118 of the
    # 128 columns a wave pair stages as `lane` and `lane + 64`
    assert lds["k3l4_a8"] == [3648, 11328, 37440, 143424] and G.layers(cfg["k3l4_a8"])[3][2] == 27
    assert G.LDS_DEFAULT < lds["k3l4_a8"][3] <= G.LDS_MAX and "k3l4_a8" in G.CROP_ROWS
    widest = max(G.TILE + 2 * d for r in G.ROWS for i, (_, _, d, _) in enumerate(G.layers(r.cfg)) if lds[r.id][i])
    assert widest == G.TILE + 2 * 27 and G.TILE < widest <= 2 * G.TILE
    # the attribute path: below, above the production request, and the last size that is staged
    assert lds["k3l3_a12"][2] == 56160 and G.LDS_DEFAULT < 56160 < G.PROD_LDS
    assert lds["k3l3_a20"][2] == 93600 > G.PROD_LDS
    assert lds["k3l3_a32"][2] == 149760 <= G.LDS_MAX < G.lds_formula(33 * 9, 9) == 154440
    assert lds["k3l3_a33"] == [15048, 46728, 0]
    assert lds["k3l3_a12"][2] < lds["k3l3_a20"][2] < lds["k3l3_a32"][2]      # the high-water mark grows at every step of HIGH_WATER
    assert [lds[i][2] for i in G.HIGH_WATER[:3]] == sorted(lds[i][2] for i in G.HIGH_WATER[:3]) and G.HIGH_WATER[3] == G.HIGH_WATER[0]
    # any other kernel size is unstaged: the generic loop (5, 7) and the ks == 1 instance
    for i, k, la, d, a0 in (("k5l3_a2", 5, 62, 25, 250), ("k5l4_a1", 5, 312, 125, 625), ("k7l1_a2", 7, 3, 1, 14),
                            ("k1l4_a5", 1, 0, 1, 5), ("k1l1_a16", 1, 0, 1, 16)):
        assert set(lds[i]) == {0} and cfg[i].aux_kernel_size == k
        assert (G.lookahead(cfg[i]), G.max_dilation(cfg[i]), cfg[i].A0) == (la, d, a0)
    for r in G.ROWS:
        want = {"staged": 0 < r.lds <= G.LDS_DEFAULT, "attribute": G.LDS_DEFAULT < r.lds <= G.LDS_MAX,
                "unstaged3": r.cfg.aux_kernel_size == 3 and lds[r.id][-1] == 0,
                "generic": r.cfg.aux_kernel_size > 3 and r.lds == 0, "k1": r.cfg.aux_kernel_size == 1 and r.lds == 0}
        assert want[r.path], r.id
    assert {r.path for r in G.ROWS} == {"staged", "attribute", "unstaged3", "generic", "k1"}
    # the rows the other checks run on exist and take different paths
    assert [G.BY_ID[i].path for i in G.CROP_ROWS] == ["staged", "attribute", "attribute", "unstaged3", "generic", "k1"]
    assert all(i in G.BY_ID for i in G.POOL_ROWS + G.MODELS_ROWS + G.STREAM_ROWS)
    for i in G.STREAM_ROWS:                                  # a DecodeStream can be opened on the rows that are streamed
        d = _lib.desc_from_cfg(cfg[i])
        assert _lib.lib().swn_decode_resolve_variant(ctypes.byref(d), 2, 0) >= 0, i


def test_gemm_edges_are_present():
    N = {r.id: G.cond_width(r.cfg) for r in G.ROWS}
    A0 = {r.id: r.cfg.A0 for r in G.ROWS}
    assert N["k3l1_a1"] == 30 and N["k3l4_a9"] == 432
    assert any(n & 3 for n in N.values())                                        # the scalar-store branch
    assert any(n & 3 and A0[i] > 64 for i, n in N.items())                       # ... also behind a long chain
    assert any(n % 4 == 0 and n % 64 != 0 and n > 64 for n in N.values())        # a partial last n-tile of several
    assert any(n & 3 and n > 64 for n in N.values())                             # ... and one stored by scalars
    assert any(n <= 64 for n in N.values()) and any(n == 64 for n in N.values())
    assert any(a < 16 for a in A0.values())                                      # the prefetch guard never fires
    assert any(a == 16 for a in A0.values()) and any(a > 16 and a % 16 == 0 for a in A0.values())
    assert any(a % 4 for a in A0.values()) and max(A0.values()) == 891           # A0p pad lanes; the longest chain
    kinds = {(r.cfg.kind, bool(r.cfg.aux_conv2d_flag and r.cfg.kind == "laplace" and r.cfg.seg > 1)) for r in G.ROWS}
    assert ("softmax", False) in kinds and ("laplace", True) in kinds and ("laplace", False) in kinds
    assert any(r.cfg.kind == "softmax" and r.cfg.audio_in_flag for r in G.ROWS)
    # the pool's tap passes: J = cin * ks on and off a multiple of FP_JB = 96, below one pass and over many
    J = {(cin * r.cfg.aux_kernel_size) for r in G.ROWS if r.id in G.POOL_ROWS for cin, _, _, _ in G.layers(r.cfg)}
    assert any(j < 96 for j in J) and any(j > 96 and j % 96 for j in J) and any(j % 96 == 0 for j in J)
    assert {G.BY_ID[i].cfg.aux_kernel_size for i in G.POOL_ROWS} == {1, 3, 5, 7}
    assert max(G.BY_ID[i].cfg.aux_dilation_size for i in G.POOL_ROWS) == 4       # five stages


@pytest.mark.parametrize("row", G.ROWS, ids=IDS)
def test_frame_counts_cover_the_tile_and_halo_edges(row):
    cfg, counts = row.cfg, G.frame_counts(row.cfg)
    d, la = G.max_dilation(cfg), G.lookahead(cfg)
    assert {63, 64, 65, 130} <= set(counts) and 1 in counts
    assert d in counts and d + 1 in counts and la + 1 in counts
    if d > 1:
        assert any(n < d for n in counts)                    # every tap of the widest layer but the centre one is padding
    assert 64 + d in counts and 65 + d in counts             # the halo crosses from the last full tile into a partial one
    assert all(n >= 1 for n in G.pool_lengths(cfg)) and 6 <= len(G.pool_lengths(cfg)) <= 7
    assert lookahead_frames(cfg) == la == sum(h for _, _, _, h in G.layers(cfg))


@pytest.mark.parametrize("row", G.ROWS, ids=IDS)
def test_size_queries_follow_the_geometry(row):
    lib, cfg = _lib.lib(), row.cfg
    d = ctypes.byref(_lib.desc_from_cfg(cfg))
    chans = cfg.n_aux + sum(cout for _, cout, _, _ in G.layers(cfg))
    assert G.layers(cfg)[-1][1] == cfg.A0
    for B in (1, 3):
        for Tf in (1, 65):
            assert lib.swn_frontend_work_floats(d, B, Tf) == B * Tf * chans
            assert lib.swn_cond_floats(d, B, Tf) == B * Tf * G.cond_width(cfg)


@pytest.mark.parametrize("row", G.ROWS, ids=IDS)
def test_fp32_oracle_stays_within_a_fixed_fraction_of_float64(row):
    """4 * e32 <= 1e-4 * scale at every stage: the inputs are sound before any kernel is involved"""
    cfg = row.cfg
    for batch, Tf in [(1, n) for n in G.frame_counts(cfg)] + [(3, 65)]:          # every shape the GPU file derives a bound at
        aux, ref, figs = G.reference(row, batch, Tf)
        assert len(ref) == cfg.aux_dilation_size + 2 and ref[-1].shape == (batch, Tf, G.cond_width(cfg))
        for what, (e32, scale) in zip(G.stage_names(cfg), figs):
            print(f"[frontend-geometry] {row.id} B {batch} Tf {Tf} {what}: e32 {e32:.2e} scale {scale:.2e} "
                  f"bound {G.bound(e32, scale):.2e}")
            assert scale > 0 and G.ORDER * e32 <= G.CAP * scale, (row.id, batch, Tf, what, e32, scale)
    # the staged activations are cpu_ref.frontend's, and utterance b of a batch is the single utterance of seed + b
    aux, ref, _ = G.reference(row, 3, 65)
    assert torch.equal(ref[-2], cpu_ref.frontend(cfg, G.params(row, torch.float64), aux.double()))
    assert torch.equal(aux[2:3], G.features(cfg, 1, 65, seed=3))
