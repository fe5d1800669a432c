"""CPU: the mel-cepstrum matrix of the package (melspec.mcep_matrix, what the operator multiplies with) against the yardstick of
tests/mcep_ref.py, which goes through no matrix (irfft, the one-sided doubling, the SPTK freqt recursion); the entry points of
the C ABI and every refusal decided before a device is touched (fake pointers: nothing is launched); the new flags of the
drivers; and the loop the feature closes on the host: statistics of a /feat_mcep dataset -> noise shaping and its inverse."""
import ctypes

import numpy as np
import pytest
import torch

import mcep_ref as MC
from shallow_wavenet_amd import _lib, dsp, featio, melspec, ops
from shallow_wavenet_amd import decode_driver as DD
from shallow_wavenet_amd import feature_extract_driver as FD
from shallow_wavenet_amd import noise_shaping_driver as ND

NEW_SYMBOLS = ("swn_mcep", "swn_mcep_table_floats", "swn_mcep_work_bytes")
# (n_fft, order, alpha): the GPU tests' geometries, the order edges, alpha 0 and a negative alpha
MATRICES = [(n, M, a) for _, n, _, M, a in MC.GEOMETRIES] + [(32, 0, 0.31), (32, 16, 0.31), (256, 24, 0.0), (128, 20, -0.2)]


@pytest.mark.parametrize("n_fft,order,alpha", MATRICES)
def test_matrix_applied_to_random_log_spectra_equals_the_recursion(n_fft, order, alpha):
    G = melspec.mcep_matrix(n_fft, order, alpha)
    assert G.shape == (order + 1, n_fft // 2 + 1) and G.dtype == np.float64
    L = np.random.default_rng(n_fft + order).normal(size=(6, n_fft // 2 + 1)) * 3.0
    want = MC.freqt(MC.one_sided_cepstrum(L, n_fft), order, alpha)
    err = np.abs(L @ G.T - want).max()
    print(f"n_fft {n_fft} order {order} alpha {alpha}: |G L - recursion| {err:.1e}, |G - reference matrix| "
          f"{np.abs(G - MC.matrix(n_fft, order, alpha)).max():.1e}")
    assert err <= 1e-12


@pytest.mark.parametrize("n_fft,order,alpha", MATRICES)
def test_matrix_properties(n_fft, order, alpha):
    G = melspec.mcep_matrix(n_fft, order, alpha)
    bins = n_fft // 2 + 1
    # a constant L maps to mc = (L, 0, ...): row 0 sums to 1, the others to 0
    assert abs(G[0].sum() - 1.0) <= 1e-13 and np.abs(G[1:].sum(axis=1)).max(initial=0.0) <= 1e-13
    # the bound of the GPU tests is tight because no row amplifies: max over rows of sum |G|
    gain = np.abs(G).sum(axis=1).max()
    print(f"n_fft {n_fft} order {order} alpha {alpha}: max row sum of |G| {gain:.3f}")
    assert gain < 1.5
    if alpha == 0.0:
        # no warping: the plain one-sided cepstrum, c[k] = e_k / n sum_b e_b L[b] cos(2 pi k b / n)
        e = np.full(bins, 2.0)
        e[0] = e[-1] = 1.0
        k, b = np.arange(order + 1)[:, None], np.arange(bins)[None, :]
        assert np.abs(G - e[:order + 1, None] * e[None, :] * np.cos(2 * np.pi * k * b / n_fft) / n_fft).max() <= 1e-15
        assert np.abs(G - MC.one_sided_cepstrum(np.eye(bins), n_fft).T[:order + 1]).max() <= 1e-15


def test_one_sided_convention_reproduces_the_amplitude():
    """|exp(sum_k c(k) z^-k)| = A on the unit circle at the bins: the convention dsp.py and the MLSA filter use"""
    n = 64
    A = np.random.default_rng(1).uniform(0.1, 3.0, n // 2 + 1)
    c = MC.one_sided_cepstrum(np.log(A), n)
    w = 2 * np.pi * np.arange(n // 2 + 1) / n
    H = np.exp(sum(c[k] * np.exp(-1j * k * w) for k in range(n // 2 + 1)))
    assert np.abs(np.abs(H) - A).max() <= 1e-12


def test_tables_layout_and_rounding():
    for n_fft, order, alpha in MATRICES:
        t = melspec.mcep_tables(n_fft, order, alpha)
        bins, kp = n_fft // 2 + 1, (n_fft // 2 + 1 + 3) & ~3
        assert t.dtype == np.float32 and t.shape == (2 * n_fft + (order + 1) * kp,)
        assert t.shape[0] == _lib.lib().swn_mcep_table_floats(n_fft, order)
        assert np.array_equal(t[:2 * n_fft], melspec.tables(8000, n_fft, 1)[0][:2 * n_fft])       # cos and window: the log-mel ones
        G = t[2 * n_fft:].reshape(order + 1, kp)
        assert np.array_equal(G[:, :bins], melspec.mcep_matrix(n_fft, order, alpha).astype(np.float32))
        # fp32 roundings of the reference's matrix (entries below 1: half an ulp is at most 2^-25) plus the float64 difference
        assert np.abs(G[:, :bins].astype(np.float64) - MC.matrix(n_fft, order, alpha)).max() <= 2.0 ** -25 + 1e-14
        assert not G[:, bins:].any()
    for bad in ((1024, -1, 0.4), (1024, 64, 0.4), (32, 17, 0.4), (1000, 10, 0.4), (1024, 10, 1.0)):
        with pytest.raises(ValueError):
            melspec.mcep_matrix(*bad)


def test_reference_fp32_evaluation_and_fma_chain():
    fs, n_fft, hop, order, alpha = MC.GEOMETRIES[1]
    import melspec_ref as MR
    x = MR.signal("broadband", 700, fs, seed=3)
    ref, r32 = MC.mcep(x, n_fft, hop, order, alpha), MC.mcep32(x, n_fft, hop, order, alpha)
    tol, e32, B = MC.tolerance(x, n_fft, hop, order, alpha)
    assert ref.shape == r32.shape == tol.shape == (1 + 700 // hop, order + 1) and r32.dtype == np.float32
    assert np.abs(r32 - ref).max() <= 1e-4 and (np.abs(r32 - ref) <= tol).all() and 0 < e32 < 1e-6
    # the chain: exact on numbers whose products and sums are exact, one rounding per step otherwise
    L = np.arange(1, 9, dtype=np.float32)
    G = np.stack([np.ones(8, dtype=np.float32), np.float32(2.0) ** -np.arange(8, dtype=np.float32)])
    assert np.array_equal(MC.fma_chain(L, G), np.array([36.0, (L * G[1]).sum()], dtype=np.float32))
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-1.0)
    assert MC.fma32(a, b, c) == np.float32(2.0 ** -11 + 2.0 ** -24)                 # a product rounded first would lose 2^-24


def test_symbols_are_exported_bound_and_registered():
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3 and _lib.MCEP_MAX_ORDER == 63
    assert "mcep" in ops.OP_NAMES
    assert str(torch.ops.swn.mcep.default._schema).startswith("swn::mcep(")


def _entry(wav=1, out=1, t0=0, n_avail=3001, length=3001, f0=0, f1=28, reserved=0):
    return _lib.LogMelEntry(wav_dev=wav or None, out_dev=out or None, t0=t0, n_avail=n_avail, len=length, f0=f0, f1=f1,
                            reserved=reserved)


def test_size_queries_return_zero_on_refused_arguments():
    lib = _lib.lib()
    assert lib.swn_mcep_table_floats(1024, 49) == 2 * 1024 + 50 * 516
    assert lib.swn_mcep_table_floats(32, 16) == 2 * 32 + 17 * 20 and lib.swn_mcep_table_floats(2048, 63) == 2 * 2048 + 64 * 1028
    assert lib.swn_mcep_table_floats(32, 0) == 2 * 32 + 20
    for n, m in ((0, 8), (16, 8), (48, 8), (2080, 8), (1024, -1), (1024, 64), (32, 17)):
        assert lib.swn_mcep_table_floats(n, m) == 0
    en = (_lib.LogMelEntry * 2)(_entry(length=3001, f1=28), _entry(length=600, n_avail=600, f1=5))
    assert lib.swn_mcep_work_bytes(1024, 110, en, 2) == 3 * 16 * 516 * 4 == lib.swn_logmel_work_bytes(1024, 110, en, 2)
    assert lib.swn_mcep_work_bytes(1024, 110, en, 0) == 0 and lib.swn_mcep_work_bytes(1024, 0, en, 2) == 0
    assert lib.swn_mcep_work_bytes(1024, 110, None, 2) == 0 and lib.swn_mcep_work_bytes(1000, 110, en, 2) == 0
    bad = (_lib.LogMelEntry * 1)(_entry(f1=29))                                  # a signal of 3 001 samples has 28 frames
    assert lib.swn_mcep_work_bytes(1024, 110, bad, 1) == 0
    assert b"swn_mcep_work_bytes" in lib.swn_last_error_detail()


def _call(n_fft=1024, hop=110, order=49, floor=1e-5, tables=1, work=1, **kw):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    table = (_lib.LogMelEntry * 1)(_entry(**kw))
    return lib.swn_mcep(n_fft, hop, order, floor, p(tables), table, 1, p(work), None), lib.swn_last_error_detail().decode()


def test_call_refuses_bad_arguments_before_any_launch():
    for kw, text in ((dict(order=-1), "order outside"), (dict(order=64), "order outside"), (dict(n_fft=32, hop=8, order=17), "n_fft / 2"),
                     (dict(floor=0.0), "floor"), (dict(floor=-1.0), "floor"), (dict(floor=float("nan")), "floor"),
                     (dict(n_fft=1000), "multiple of 32"), (dict(hop=0), "hop"), (dict(f1=29), "28 frames"),
                     (dict(reserved=1), "reserved"), (dict(wav=0), "null pointer"), (dict(tables=0), "null pointer"),
                     (dict(work=0), "null pointer"), (dict(n_avail=3000), "window")):
        rc, detail = _call(**kw)
        assert rc == -2 and detail.startswith("swn_mcep: ") and text in detail, (kw, rc, detail)
    assert _call(f0=5, f1=5, wav=0, out=0, tables=0, work=0)[0] == 0              # no frame: nothing is launched
    # the refusals of the Python layers
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.mcep_impl(torch.zeros(1, 3001), torch.zeros(2048 + 50 * 516), [0], [3001], [3001], [0], [28], 1024, 110, 49, 1e-5)
    for kw in (dict(order=64), dict(order=-1), dict(floor=0.0), dict(hop=0), dict(n_fft=1000), dict(alpha=1.0)):
        args = dict(fs=22050, n_fft=1024, hop=110, order=49, alpha=0.455, floor=1e-5, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError):
            melspec.MelCepstrumExtractor(**args)


class _FakeOp:
    """stands in for ops.mcep_impl: records the call, checks it against the C call's rules, returns frame indices"""

    def __init__(self):
        self.calls = []

    def __call__(self, wav, tables, t0s, n_avails, lens, f0s, f1s, n_fft, hop, order, floor):
        self.calls.append((tuple(wav.shape), t0s, n_avails, lens, f0s, f1s))
        for r in range(wav.shape[0]):
            en = (_lib.LogMelEntry * 1)(_entry(t0=t0s[r], n_avail=n_avails[r], length=lens[r], f0=f0s[r], f1=f1s[r]))
            assert _lib.lib().swn_mcep_work_bytes(n_fft, hop, en, 1) > 0, _lib.lib().swn_last_error_detail().decode()
        assert tables.numel() == _lib.lib().swn_mcep_table_floats(n_fft, order)
        return torch.zeros((wav.shape[0], max(b - a for a, b in zip(f0s, f1s)), order + 1))


def test_extractor_call_forms_with_a_fake_operator():
    ext = melspec.MelCepstrumExtractor(8000, 64, 16, 12, 0.31, device="cpu")
    ext._op = _FakeOp()
    assert ext.frame_count(1000) == 63
    assert ext(torch.zeros(1000)).shape == (1, 63, 13)
    assert ext([torch.zeros(1000), torch.zeros(500)]).shape == (2, 63, 13)
    assert ext(torch.zeros(2, 1000), lengths=[1000, 640]).shape == (2, 63, 13)
    assert ext._op.calls[-1][1:] == ([0, 0], [1000, 640], [1000, 640], [0, 0], [63, 41])
    assert ext.frames(torch.zeros(200), 100, 200, -1, 9, 15).shape == (6, 13)
    assert ext.frames(torch.zeros(2, 1000), 0, 1000, 1000, [0, 3], [63, 9]).shape == (2, 63, 13)
    with pytest.raises(ValueError, match="longer than"):
        ext(torch.zeros(32))


def test_driver_flags_parse():
    a = FD.build_parser().parse_args([])
    assert (a.mcep_dim, a.mcep_alpha, a.mcep_floor, a.mcep_string_path, a.feature_type) == (0, 0.455, 1e-5, "/feat_mcep", "logmel")
    a = FD.build_parser().parse_args(["--feature_type", "mcep", "--mcep_dim", "24", "--mcep_alpha", "0.41", "--mcep_floor", "1e-4",
                                      "--mcep_string_path", "/mc"])
    assert (a.mcep_dim, a.mcep_alpha, a.mcep_floor, a.mcep_string_path, a.feature_type) == (24, 0.41, 1e-4, "/mc", "mcep")
    a = ND.build_parser().parse_args([])
    assert a.stats_string_path == "/feat_org_lf0" and a.mcep_dim_start == 5
    a = ND.build_parser().parse_args(["--stats_string_path", "/feat_mcep", "--mcep_dim_start", "0"])
    assert a.stats_string_path == "/feat_mcep" and a.mcep_dim_start == 0
    need = ["--feats", "f", "--checkpoint", "c", "--config", "g", "--outdir", "o"]
    assert DD.make_parser().parse_args(need).stats_string_path == "/feat_org_lf0"
    assert DD.make_parser().parse_args(need + ["--stats_string_path", "/feat_mcep"]).stats_string_path == "/feat_mcep"
    for parser, flag in ((FD.build_parser(), "mcep_floor"), (FD.build_parser(), "mcep_string_path"),
                         (ND.build_parser(), "stats_string_path"), (DD.make_parser(), "stats_string_path")):
        assert "not a reference flag" in next(x.help for x in parser._actions if x.dest == flag)


def test_mcep_statistics_drive_the_noise_shaping_round_trip(tmp_path):
    """statistics of a /feat_mcep dataset (c(0) first: mcep_dim_start 0) -> mean_mcep_vector -> shaping (inv) and restoring: the
    identity up to the two 70 Hz low cuts, within the tolerance tests/test_dsp.py uses for that round trip"""
    fs, order, alpha = 22050, 12, 0.455
    rng = np.random.default_rng(0)
    t = np.arange(fs // 2) / fs
    x = 0.25 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.standard_normal(t.size)
    # mel-cepstra of the reference on this waveform stand in for a corpus: two feature files, then calc_stats
    mc = MC.mcep(x.astype(np.float32), 512, 110, order, alpha)
    files = []
    for i, part in enumerate((mc[:40], mc[40:])):
        files.append(str(tmp_path / f"utt{i}.npz"))
        featio.write_dataset(files[-1], "/feat_mcep", part.astype(np.float32))
    mean, scale = featio.calc_stats(files, "/feat_mcep")
    stats = str(tmp_path / "stats.npz")
    featio.write_stats(stats, "/feat_mcep", mean, scale)
    got = ND.mean_mcep_vector(stats, "/feat_mcep")
    assert got.shape == (order + 1,) and np.allclose(got, mc.astype(np.float32).mean(axis=0), atol=1e-6)
    with pytest.raises(KeyError):
        ND.mean_mcep_vector(stats)                                           # the default still looks for /mean_org_lf0
    shaped = dsp.noise_shaping(x, got, fs, alpha, mcep_dim_start=0, inv=True)
    assert np.max(np.abs(shaped[300:] - x[300:])) > 1e-2                     # it did something
    back = dsp.noise_shaping(shaped, got, fs, alpha, mcep_dim_start=0, inv=False)
    d = 254                                                                  # two 255-tap linear-phase low cuts
    ref = x[: x.size - d]
    err = back[d:] - ref
    assert np.sqrt(np.mean(err[2000:] ** 2)) < 0.02 * np.sqrt(np.mean(ref[2000:] ** 2)) + 1e-3
    # the default string path reads today's file as before
    full = np.concatenate([[0.9, 5.0, -3.0, -4.0, 0.1], got])
    featio.write_stats(stats, "/feat_org_lf0", full, np.ones_like(full))
    assert np.array_equal(ND.mean_mcep_vector(stats), full)
