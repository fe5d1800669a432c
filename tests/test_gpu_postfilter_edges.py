"""GPU: the device noise-shaping post-filter (swn_postfilter_chunk through torch.ops.swn.postfilter_chunk) against the exact
references of tests/postfilter_ref.py, at the filter shapes where a kernel that keeps chain element k in lane k can go wrong.

The filter image [b | taps | mu-law table] is built here, so any order, alpha and tap set runs: orders 1, 2, 3 (no or one chain
lane), 31 / 32 / 33 (the edge of a scan step), 61 / 62 (the top lanes; lane 63 must contribute exact zeros), alpha <= 0
(p = -alpha vanishes or changes sign), 1, 2, 64, 65, 255 and 256 taps, and chunks shorter than the FIR history at a tile edge.

Bound per sample (derived in postfilter_ref, not fitted):  |y - ref| <= 2^-24 |ref| (1 + 2^-20) + E64,  E64 = 2^-52 K L1 max|x|.
The saved state is held to E64 / max|x| times the scale of its section, and a slot resumed from a state uploaded from the
reference must continue within the output bound: that pins the documented layout, not the kernel's agreement with itself.

Mutants of csrc/swn_postfilter.hip.  Deliberately wrong kernels are not run on a device: each mutant was applied to a float64
numpy transcription of the kernel, statement by statement with the 64 lanes as an array axis (the unmutated transcription passes
every check below on the CPU), and that was run through the checks of this file and through the criteria of
test_gpu_postfilter.py as it stood before this change (order 49 only: 1e-6 against the host code, chunks bitwise).  x / 17 is the
number of grid cases of test_lengths_state_and_resume that fail; `old` says whether the older file fails too.

    Bk loop bound `i >= k` -> `i > k`                outputs, state and resumed run 12 / 17 (every order >= 3)         old: yes
    the final `G *= p` dropped                       outputs, state and resumed run 14 / 17 (every order >= 2)         old: yes
    `keep` cut to `k < m`                            state 17 / 17 (at order 1 only the state shows it), outputs and
                                                     resumed run 12 / 17                                               old: yes
    history copy reading `lw[cnt + i - 1]`           outputs and state 15 / 17 (every case with taps >= 2), and
                                                     test_chunked_equals_one_shot_bitwise at every cut                 old: yes
    `pw` started at p instead of 1                   state 17 / 17, outputs and resumed run 14 / 17 (orders >= 2)      old: yes
    output scaled by 1 + 4e-7                        outputs and resumed run 17 / 17; the state is untouched           old: no
    `sec[k + 1]` as `sec[k]` on load and store       state 17 / 17, resumed run 14 / 17 (orders >= 2); outputs and
                                                     chunking agree with themselves and pass                           old: no
    scan step `k >= off` -> `k > off`                equivalent, no test can fail: lane k = off would add P S[0], and
                                                     S[0] (lane 0: no chain element, never added to) is exactly 0.0
"""
import numpy as np
import pytest
import torch

import postfilter_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_OP = None


def _op():
    global _OP
    if _OP is None:
        from shallow_wavenet_amd import ops  # noqa: F401  (registers torch.ops.swn.*)
        _OP = torch.ops.swn.postfilter_chunk
    return _OP


def _image(c, q=None):
    parts = [c.b, c.taps] + ([R.mulaw_table(q)] if q else [])
    return torch.from_numpy(np.concatenate(parts)).to(DEV)


def _garbage(c, capacity, seed=0):
    """a state nobody wrote: a reset must not read it, a run without reset would show it"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(capacity * R.state_doubles(c.order, c.pade, c.n_taps), generator=g, dtype=torch.float64).to(DEV)


def _call(c, image, state, xs, slots, resets, capacity):
    out = _op()(image, state, xs, list(slots), list(resets), c.order, c.alpha, c.pade, c.n_taps, capacity)
    return [out[e, :x.numel()] for e, x in enumerate(xs)]


def _share(got, ref, e):
    """worst |got - ref| as a share of the bound, and the worst share among the samples where E64 is over a tenth of the bound"""
    if got.size == 0:
        return 0.0, 0.0
    bound = R.output_bound(ref, e)
    s = np.abs(got.astype(np.float64) - ref) / bound
    near0 = e > 0.1 * bound
    return float(s.max()), float(s[near0].max()) if near0.any() else 0.0


_RUNS = {}


def _case_run(name):
    """one case's device results: the nine lengths in one call (three signals' prefixes), the slot state after the longest,
    and signal 2 continued in a slot whose state was uploaded from the reference."""
    if name in _RUNS:
        return _RUNS[name]
    c = R.case(name)
    img = _image(c)
    x = torch.from_numpy(c.x).to(DEV)
    E = len(R.LENGTHS)
    per = R.state_doubles(c.order, c.pade, c.n_taps)
    state = torch.full(((E + 1) * per,), float("nan"), dtype=torch.float64, device=DEV)   # a reset reads nothing of it
    xs = [x[e % 3, :n] for e, n in enumerate(R.LENGTHS)]
    ys = _call(c, img, state, xs, range(E), [True] * E, E + 1)
    after = state.view(E + 1, per).cpu().numpy().copy()
    assert (E - 1) % 3 == 2 and R.LENGTHS[-1] == R.N_LONG                                 # the longest entry is signal 2
    state.view(E + 1, per)[E] = torch.from_numpy(c.long_run[1][2]).to(DEV)
    cont = _call(c, img, state, [x[2, R.N_LONG:]], [E], [False], E + 1)[0]
    _RUNS[name] = dict(ys=[y.cpu().numpy() for y in ys], state=after[E - 1], untouched=after[E], cont=cont.cpu().numpy())
    return _RUNS[name]


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_lengths_state_and_resume(gpu_ok, name):
    c = R.case(name)
    r = _case_run(name)
    yref, sref = c.long_run
    # ---- outputs of every length
    worst = (0.0, 0.0)
    for e, n in enumerate(R.LENGTHS):
        got, ref = r["ys"][e], yref[e % 3, :n]
        assert got.dtype == np.float32 and got.shape == (n,)
        xmax = float(np.abs(c.x[e % 3, :n]).max())
        s = _share(got, ref, c.e64(xmax))
        worst = (max(worst[0], s[0]), max(worst[1], s[1]))
        print(f"{name} n {n}: share of the bound {s[0]:.3f}  near zero {s[1]:.3g}")
    cont_share = _share(r["cont"], c.resumed, c.e64(float(np.abs(c.x[2]).max())))
    print(f"{name} resumed from the reference's state: share {cont_share[0]:.3f}  near zero {cont_share[1]:.3g}")
    # ---- the slot's state after N_LONG samples, section by section
    tol = c.e64(1.0)                                                                      # E64 / max|x|
    shares = []
    for sec_name, got, ref in zip(("stage 1", "stage 2", "history"), R.state_sections(r["state"], c.order, c.pade, c.n_taps),
                                  R.state_sections(sref[2], c.order, c.pade, c.n_taps)):
        if ref.size == 0:
            continue
        scale = float(np.abs(ref).max())
        assert scale > 0.0
        shares.append((sec_name, float(np.abs(got - ref).max()) / (tol * scale)))
        print(f"{name} state {sec_name}: share of its tolerance {shares[-1][1]:.3g}  (scale {scale:.3g})")
    assert np.isnan(r["untouched"]).all()                                                 # a slot no entry named
    assert worst[0] <= 1.0, (name, worst)
    assert all(s <= 1.0 for _, s in shares), (name, shares)
    assert np.isfinite(r["state"]).all()
    assert r["cont"].shape == (R.N_RESUME,) and cont_share[0] <= 1.0, (name, cont_share)
    assert float(np.abs(yref[2]).max()) > 0.05                                            # it filtered something


CHUNK_CASES = ["m1-p4-one", "m1-p5-a0-two", "m2-p4-lowcut", "m32-p4-lowcut", "m33-p4-aneg-two", "m33-p5-a0-r64",
               "m62-p4-aneg-lowcut", "m62-p5-r256"]
CUTS = (1, 253, 254, 255, 256, 511, 512, 513, 1024, 1025)


def _chunk_case(name):
    """the grid's cases at the edge orders; the two- and 255-tap sets are forced where the grid's own taps differ"""
    c = R.case(name)
    if c.n_taps in (2, 255):
        return c
    d = R.Case(name)
    d.taps = R.low_cut_255() if c.order != 1 else np.array([0.75, -0.25])
    d.n_taps = d.taps.size
    return d


@pytest.mark.parametrize("name", CHUNK_CASES)
def test_chunked_equals_one_shot_bitwise(gpu_ok, name):
    c = _chunk_case(name)
    assert c.n_taps in (2, 255)
    img = _image(c)
    x = torch.from_numpy(c.x[0, :R.N_LONG]).to(DEV)
    n = x.numel()
    splits = {cut: [0, cut, n] for cut in CUTS}
    splits["ones"] = list(range(601))                                                     # chunk size 1 over 600 samples
    cap = len(splits) + 1
    state = _garbage(c, cap)
    whole = _call(c, img, state, [x], [cap - 1], [True], cap)[0]
    slots = {k: i for i, k in enumerate(splits)}
    got = {k: [] for k in splits}
    pos = {k: 0 for k in splits}
    while any(pos[k] < len(splits[k]) - 1 for k in splits):       # every split advances in the same calls
        live = [k for k in splits if pos[k] < len(splits[k]) - 1]
        xs = [x[splits[k][pos[k]]:splits[k][pos[k] + 1]] for k in live]
        out = _call(c, img, state, xs, [slots[k] for k in live], [pos[k] == 0 for k in live], cap)
        for k, y in zip(live, out):
            got[k].append(y)
            pos[k] += 1
    for k in splits:
        cat = torch.cat(got[k])
        assert torch.equal(cat, whole[:cat.numel()]), (name, k)
    assert torch.cat(got["ones"]).numel() == 600 and float(whole.abs().max()) > 0.05


@pytest.mark.parametrize("E", [65, 129])
def test_more_than_one_launch_group(gpu_ok, E):
    name = "m31-p5-r65"
    c = R.case(name)
    img = _image(c)
    x = torch.from_numpy(c.x).to(DEV)
    rng = np.random.default_rng(E)
    checked = {0: 513, 63: 1, 64: 767, 128: 897}                                          # entry -> its length
    checked = {e: n for e, n in checked.items() if e < E}
    lengths = rng.permutation([n for n in range(2, 900) if n not in checked.values()])[:E].tolist()
    for e, n in checked.items():
        lengths[e] = n
    assert len(set(lengths)) == E                                                         # distinct
    z_reset, z_keep = 7, 40                                                               # the two empty entries
    lengths[z_reset] = lengths[z_keep] = 0
    per = R.state_doubles(c.order, c.pade, c.n_taps)
    state = _garbage(c, E, seed=E)
    before = state.view(E, per)[z_keep].clone()
    xs = [x[e % 3, :n] for e, n in enumerate(lengths)]
    resets = [e != z_keep for e in range(E)]
    ys = _call(c, img, state, xs, range(E), resets, E)
    assert torch.equal(state.view(E, per)[z_keep], before)                                # n = 0 without reset: not a bit moves
    yref = c.long_run[0]
    for e in checked:
        solo = _call(c, img, _garbage(c, 1, seed=e), [xs[e]], [0], [True], 1)[0]
        assert torch.equal(ys[e], solo), e
        s = _share(ys[e].cpu().numpy(), yref[e % 3, :lengths[e]], c.e64(float(np.abs(c.x[e % 3, :lengths[e]]).max())))
        print(f"E {E} entry {e} n {lengths[e]}: share of the bound {s[0]:.3f}  near zero {s[1]:.3g}")
        assert s[0] <= 1.0, (E, e, s)
    # n = 0 with reset cleared its slot: the next run without reset is a fresh run
    again = _call(c, img, state, [x[1, :300]], [z_reset], [False], E)[0]
    fresh = _call(c, img, _garbage(c, 1, seed=99), [x[1, :300]], [0], [True], 1)[0]
    assert torch.equal(again, fresh)


@pytest.mark.parametrize("q", [256, 90])
def test_mulaw_classes_outside_the_table_are_clamped(gpu_ok, q):
    c = R.case("m49-p4-lowcut")
    rng = np.random.default_rng(q)
    classes = rng.integers(0, q, 520).astype(np.int64)
    special = np.array([-1, -2 ** 31, 0, q - 1, q, 255, 256, 1000, 2 ** 31 - 1], dtype=np.int64)
    classes[rng.permutation(520)[:special.size]] = special
    classes[:3] = [-2 ** 31, 2 ** 31 - 1, -1]
    xq = torch.from_numpy(classes.astype(np.int32)).to(DEV)
    got = _call(c, _image(c, q), _garbage(c, 1), [xq], [0], [True], 1)[0].cpu().numpy()
    xd = R.mulaw_decode(classes, q)
    assert np.array_equal(xd, R.mulaw_table(q)[np.clip(classes, 0, min(q - 1, 255))])
    ref, _ = R.restore_ref(xd, *c.args)
    s = _share(got, ref, c.e64(float(np.abs(xd).max())))
    print(f"mu-law Q {q}: share of the bound {s[0]:.3f}  near zero {s[1]:.3g}")
    assert s[0] <= 1.0, (q, s)


def test_input_views_off_the_16_byte_grid(gpu_ok):
    c = R.case("m49-p4-lowcut")
    img = _image(c)
    base = torch.from_numpy(c.x[0]).to(DEV)
    v1, v3 = base[1:1 + 1537], base[3:3 + 513]
    assert v1.is_contiguous() and v1.data_ptr() % 16 == 4 and v3.data_ptr() % 16 == 12
    xs = [v1, v1.clone(), v3, v3.clone()]
    assert xs[1].data_ptr() % 16 == 0 and xs[3].data_ptr() % 16 == 0
    ys = _call(c, img, _garbage(c, 4), xs, range(4), [True] * 4, 4)
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[2], ys[3])
    assert float(ys[0].abs().max()) > 0.05


def test_order_63_is_refused_and_order_62_runs(gpu_ok):
    c = R.case("m62-p5-a0-r65")
    d = R.Case("m62-p5-a0-r65")
    d.order, d.b = 63, np.concatenate([c.b, [0.01]])
    x = torch.from_numpy(c.x[0, :100]).to(DEV)
    state = _garbage(d, 1)
    before = state.clone()
    with pytest.raises(RuntimeError, match="not supported"):
        _call(d, _image(d), state, [x], [0], [True], 1)
    torch.cuda.synchronize()
    assert torch.equal(state, before)
    y = _call(c, _image(c), _garbage(c, 1), [x], [0], [True], 1)[0]
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0.01
