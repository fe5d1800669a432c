"""CPU: the host packer (swn_pack_params) at geometries with real padding - H, S, the out_1 width and A0 not multiples
of 4 (the g10 fixtures' nets).  The kernels read whole Hp / Sp / O1p / A0p rows, so a pad lane that is not zero is added
into every product: each padded section of the packed buffer is rebuilt here from the source tensors with numpy and
compared bit for bit - every pad position (enumerated from swn_layout_offsets and the geometry, the gap up to the next
section included) must be an exact zero and every real position the source weight itself."""
import numpy as np
import pytest

from conftest import golden_names, load_golden
from shallow_wavenet_amd.runtime import layout_offsets, pack_state_dict
from shallow_wavenet_amd.synth import synth_state_dict

G10 = golden_names("g10_odd_")
r4 = lambda x: (x + 3) & ~3


def _geom(cfg):
    seg = cfg.seg if cfg.kind == "laplace" else 1
    return dict(H=cfg.H, Hp=r4(cfg.H), S=cfg.S, Sp=r4(cfg.S), O1=cfg.out1_chn, O1p=r4(cfg.out1_chn), NO=cfg.n_out,
                A0=cfg.A0, A0p=r4(cfg.A0), K=cfg.K, L=cfg.L, seg=seg)


def _packed(name):
    cfg, d = load_golden(name)
    sd = synth_state_dict(cfg, seed=int(d["wseed"]), flavor=str(d["flavor"]))
    return cfg, sd, pack_state_dict(cfg, sd).numpy(), layout_offsets(cfg)


def _sections(cfg, sd):
    """name -> (padded array in the packed layout, name of the section that follows it)"""
    g = _geom(cfg)
    H, Hp, S, Sp, O1, O1p, NO, A0, A0p, K, L, seg = (g[k] for k in ("H", "Hp", "S", "Sp", "O1", "O1p", "NO", "A0", "A0p", "K", "L", "seg"))
    wd = np.zeros((L, 2 * H, K, Hp), np.float32)          # [l][o][k][i] = dil_h.l.conv.weight[o][i][k]
    wsk = np.zeros((S, L, Hp), np.float32)                # [c][l][i] = out_skip.l.weight[c][i]
    for l in range(L):
        wd[l, :, :, :H] = sd[f"dil_h.{l}.conv.weight"].transpose(0, 2, 1)
        wsk[:, l, :H] = sd[f"out_skip.{l}.weight"][:, :, 0]
    w1 = np.zeros((O1, Sp), np.float32)
    w1[:, :S] = sd["out_1.weight"][:, :, 0]
    w2 = np.zeros((NO, O1p), np.float32)
    w2[:, :O1] = sd["out_2.weight"][:, :, 0]
    wx = np.zeros((L, seg, 2 * H, A0p), np.float32)       # [l][s][o][c] = in_x.l.weight[o][c*seg+s] (Conv2d folded in)
    conv2d = cfg.kind == "laplace" and cfg.aux_conv2d_flag and cfg.seg > 1
    for l in range(L):
        w = sd[f"in_x.{l}.weight"][:, :, 0]
        if conv2d:
            eff = np.einsum("op,pcs->ocs", w.astype(np.float64), sd["aux_conv2d.weight"][:, :, :, 0].astype(np.float64))
        else:
            eff = w[:, : A0 * seg].reshape(2 * H, A0, seg)
        wx[l, :, :, :A0] = np.transpose(eff, (2, 0, 1))
    nxt = dict(wd="bd", wsk="bsk", w1="b1", w2="b2", wx="wxa" if cfg.kind == "softmax" and cfg.audio_in_flag else "wup")
    return dict(wd=wd, wsk=wsk, w1=w1, w2=w2, wx=wx), nxt, conv2d


def test_the_cases_have_every_kind_of_padding():
    geoms = [_geom(load_golden(n)[0]) for n in G10]
    assert len(G10) == 8
    for a, b in (("H", "Hp"), ("S", "Sp"), ("O1", "O1p"), ("A0", "A0p")):
        assert any(g[a] != g[b] for g in geoms), a
    assert any(g["NO"] % 4 for g in geoms)


@pytest.mark.parametrize("name", G10)
def test_pad_positions_are_exact_zeros(name):
    cfg, sd, packed, off = _packed(name)
    sections, nxt, _ = _sections(cfg, sd)
    n_pads = 0
    for sec, want in sections.items():
        lo, hi = off[sec], off[nxt[sec]]
        assert hi - lo >= want.size and (hi - lo) - want.size < 64, (name, sec)        # 64-float section alignment
        got = packed[lo:hi]
        pad = np.ones(hi - lo, bool)
        real = np.zeros(want.shape, bool)
        real[..., : {"wd": cfg.H, "wsk": cfg.H, "w1": cfg.S, "w2": cfg.out1_chn, "wx": cfg.A0}[sec]] = True
        pad[: want.size] = ~real.ravel()
        n_pads += int(pad.sum())
        # exact zeros: the bit pattern, so -0.0 or a denormal does not pass either
        assert not got[pad].view(np.uint32).any(), (name, sec, np.flatnonzero(got[pad].view(np.uint32))[:8])
    assert n_pads > 0


@pytest.mark.parametrize("name", G10)
def test_real_positions_hold_the_source_weights(name):
    cfg, sd, packed, off = _packed(name)
    sections, nxt, conv2d = _sections(cfg, sd)
    for sec, want in sections.items():
        got = packed[off[sec]: off[sec] + want.size].reshape(want.shape)
        for l in {0, cfg.L - 1} if sec in ("wd", "wsk", "wx") else {None}:
            g, w = (got, want) if l is None else ((got[:, l], want[:, l]) if sec == "wsk" else (got[l], want[l]))
            if sec == "wx" and conv2d:
                # folded through the (seg,1) Conv2d in double and rounded once: numpy's sum order may differ in the last bit
                assert np.abs(g - w).max() <= 2e-7 * max(1.0, np.abs(w).max()), (name, sec, l)
            else:
                assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, sec, l)
