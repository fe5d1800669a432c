"""numpy references of the device noise-shaping post-filter (swn_postfilter_chunk, include/swn_hip.h).  Nothing here imports or
restates project code: the filter is written from its published definition (Imai, Sumita, Furuichi 1983; SPTK's mlsadf).

With constant coefficients b[0 .. m], all-pass constant a and the Pade table pp of order pd the filter is LTI.  Per sample:

    stage 1   v_i = b[1] Phi1 applied i times to pt[0],  pt[0] = g x + sum_i -(-1)^i pp[i] v_i,  out = pt[0] + sum_i pp[i] v_i
    stage 2   the same around F2 = sum_{k=2..m} b[k] Phi1 A^(k-1) in place of b[1] Phi1
    FIR       y[t] = sum_q taps[q] w[t - q]

with g = exp(b[0]), Phi1 = (1 - a^2) z1 / (1 - a z1), A = (z1 - a) / (1 - a z1), z1 one sample of delay.  Every section carries
its own sample of delay (it reads the previous sample's pt[i - 1]), so the closed form is

    H(w) = exp(b[0]) P(F1) / P(-F1) P(F2) / P(-F2) H_fir(w),   P(v) = sum_i pp[i] v^i,  F1 = b[1] Phi1      (`transfer_function`)

`restore_ref` is the serial definition in np.longdouble, the all-pass chain in its textbook form: element k of a section is
n_k[t] = n_{k-1}[t-1] + a (n_k[t-1] - n_{k-1}[t]), one element after the other.  It splits nothing off and scans nothing.
Its state has the layout include/swn_hip.h documents for a session slot:

    [stage 1: d[0 .. pd] | pt[0 .. pd]]  [stage 2: pd sections of (u, n_1, n_1 .. n_m) | pt[0 .. pd]]  [the last n_taps - 1 MLSA
    outputs, oldest first]

`E64` is the fp64 term of the device bound:  2^-52 K L1 max|x|  with K = pd (4 m + 12) + n_taps + 8 the roundings one output
passes through and L1 = sum_t |h[t]| of the whole filter (`impulse_l1`)."""
import numpy as np

LD = np.longdouble
IMPULSE_N = 4096

# SPTK's published modified Pade tables of exp(), orders 4 and 5
PADE = {4: (1.0, 4.999273e-1, 1.067005e-1, 1.170221e-2, 5.656279e-4),
        5: (1.0, 4.999391e-1, 1.107098e-1, 1.369984e-2, 9.564853e-4, 3.041721e-5)}


def mc2b(mc, alpha):
    """mel-cepstrum -> filter coefficients: b[m] = c[m], b[k] = c[k] - alpha b[k + 1]"""
    b = np.array(mc, dtype=np.float64)
    for k in range(b.size - 2, -1, -1):
        b[k] = b[k] - alpha * b[k + 1]
    return b


def state_doubles(order, pade, n_taps):
    return 2 * (pade + 1) + pade * (order + 2) + pade + 1 + (n_taps - 1)


def transfer_function(b, alpha, pade, taps, n):
    """H on the n // 2 + 1 bins of an n-point rfft, complex128"""
    b, taps = np.asarray(b, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    pp = PADE[pade]
    m = b.size - 1
    z1 = np.exp(-2j * np.pi * np.arange(n // 2 + 1) / n)
    phi1 = (1.0 - alpha * alpha) * z1 / (1.0 - alpha * z1)
    ap = (z1 - alpha) / (1.0 - alpha * z1)
    f1 = b[1] * phi1
    f2 = np.zeros_like(z1)
    for k in range(m, 1, -1):                        # sum_{k=2..m} b[k] A^(k-1), Horner from the top
        f2 = (f2 + b[k]) * ap
    f2 = f2 * phi1

    def pade_ratio(f):
        num = sum(pp[i] * f ** i for i in range(pade + 1))
        den = sum(pp[i] * (-f) ** i for i in range(pade + 1))
        return num / den

    hfir = sum(taps[q] * z1 ** q for q in range(taps.size))
    return np.exp(b[0]) * pade_ratio(f1) * pade_ratio(f2) * hfir


def restore_ref(x, b, alpha, pade, taps, state=None, state_dtype=np.float64):
    """x: (n,) or (batch, n) samples; each row is filtered on its own from `state` ((S,) / (batch, S); None: zero)
    -> (y, state) as float64, of x's leading shape.  Rows only share the Python loop: no arithmetic crosses them.
    The state is returned as float64, to be compared with a device slot or uploaded to one.  That rounds it: a run resumed from
    it is the one-shot run only to ~2^-64.  state_dtype=np.longdouble returns the state unrounded (same layout, its float64
    rounding is the default's return); resumed from that, the run is the one-shot run exactly."""
    x = np.asarray(x, dtype=np.float64)
    single = x.ndim == 1
    xs = np.atleast_2d(x).astype(LD)
    nb, n = xs.shape
    b = np.asarray(b, dtype=np.float64).astype(LD)
    h = np.asarray(taps, dtype=np.float64).astype(LD)
    pd, m, nt = int(pade), b.size - 1, h.size
    pp = np.array(PADE[pd], dtype=np.float64).astype(LD)
    a = LD(np.float64(alpha))
    one_a2 = LD(1) - a * a
    gain = np.exp(b[0])
    sign = np.array([0] + [1 if i & 1 else -1 for i in range(1, pd + 1)], dtype=LD)
    S = state_doubles(m, pd, nt)
    st = np.zeros((nb, S), dtype=LD) if state is None else np.atleast_2d(np.asarray(state)).astype(LD)
    assert st.shape == (nb, S), (st.shape, (nb, S))

    o2 = 2 * (pd + 1)
    oh = o2 + pd * (m + 2) + pd + 1
    d1 = st[:, 0:pd + 1].copy()                                      # stage 1 sections' Phi1 state (d1[:, 0] is not used)
    pt1 = st[:, pd + 1:o2].copy()
    sec = st[:, o2:o2 + pd * (m + 2)].reshape(nb, pd, m + 2).copy()
    u_last = sec[:, :, 0].copy()
    N = [None, sec[:, :, 1].copy()] + [sec[:, :, k + 1].copy() for k in range(2, m + 1)]   # N[k]: (nb, pd), k = 1 .. m
    pt2 = st[:, oh - (pd + 1):oh].copy()
    w = np.concatenate([st[:, oh:], np.zeros((nb, n), dtype=LD)], axis=1)                   # history | this call's MLSA outputs
    y = np.zeros((nb, n), dtype=LD)
    hrev = h[::-1].copy()

    for t in range(n):
        # stage 1: section i filters the previous sample's pt1[i - 1]
        d1[:, 1:] = one_a2 * pt1[:, :-1] + a * d1[:, 1:]
        v = d1[:, 1:] * b[1]
        pt1[:, 1:] = v
        pt1[:, 0] = gain * xs[:, t] + (v * (pp[1:] * sign[1:])).sum(axis=1)
        s1 = pt1[:, 0] + (v * pp[1:]).sum(axis=1)
        # stage 2: section i filters the previous sample's pt2[i - 1] through Phi1 and then the all-pass chain, element by element
        u = pt2[:, :-1].copy()
        old_below = N[1]
        N[1] = one_a2 * u + a * N[1]
        acc = np.zeros((nb, pd), dtype=LD)
        for k in range(2, m + 1):
            old = N[k]
            N[k] = old_below + a * (old - N[k - 1])
            acc = acc + b[k] * N[k]
            old_below = old
        u_last = u
        pt2[:, 1:] = acc
        pt2[:, 0] = s1 + (acc * (pp[1:] * sign[1:])).sum(axis=1)
        w[:, nt - 1 + t] = pt2[:, 0] + (acc * pp[1:]).sum(axis=1)
        # FIR: y[t] = sum_q h[q] w[t - q]
        y[:, t] = (w[:, t:t + nt] * hrev).sum(axis=1)

    out = np.zeros((nb, S), dtype=LD)
    out[:, 0:pd + 1] = d1
    out[:, pd + 1:o2] = pt1
    sec = np.zeros((nb, pd, m + 2), dtype=LD)
    sec[:, :, 0] = u_last
    sec[:, :, 1] = N[1]
    for k in range(1, m + 1):
        sec[:, :, k + 1] = N[k]
    out[:, o2:o2 + pd * (m + 2)] = sec.reshape(nb, -1)
    out[:, oh - (pd + 1):oh] = pt2
    out[:, oh:] = w[:, n:]
    y64, s64 = y.astype(np.float64), out.astype(state_dtype)
    return (y64[0], s64[0]) if single else (y64, s64)


def state_sections(state, order, pade, n_taps):
    """the three documented sections of one slot's state: (stage 1, stage 2, FIR history)"""
    o2 = 2 * (pade + 1)
    oh = o2 + pade * (order + 2) + pade + 1
    assert state.shape[-1] == oh + n_taps - 1
    return state[..., :o2], state[..., o2:oh], state[..., oh:]


def impulse_response(b, alpha, pade, taps):
    x = np.zeros(IMPULSE_N)
    x[0] = 1.0
    return restore_ref(x, b, alpha, pade, taps)[0]


def impulse_l1(b, alpha, pade, taps, h=None):
    """(sum_t |h[t]|, max |h| over the last 64 samples) of the reference's own IMPULSE_N-sample impulse response"""
    h = impulse_response(b, alpha, pade, taps) if h is None else h
    return float(np.abs(h).sum()), float(np.abs(h[-64:]).max())


def roundings(order, pade, n_taps):
    """K: the fp64 roundings one output sample passes through"""
    return pade * (4 * order + 12) + n_taps + 8


def e64(order, pade, n_taps, l1, xmax):
    return 2.0 ** -52 * roundings(order, pade, n_taps) * l1 * xmax


def output_bound(y_ref, e):
    """per sample: one round-to-nearest fp32 store of the fp64 result, and the fp64 work"""
    return 2.0 ** -24 * np.abs(y_ref) * (1.0 + 2.0 ** -20) + e


def mulaw_table(q):
    """the 256-entry class -> sample table of q classes in float64: (c - 0.5) / (q - 1) * 2 - 1 expanded by mu = q - 1; entries
    from q upward hold class q - 1's value"""
    mu = q - 1
    c = np.minimum(np.arange(256, dtype=np.float64), q - 1)
    fx = (c - 0.5) / mu * 2.0 - 1.0
    return np.sign(fx) / mu * ((1.0 + mu) ** np.abs(fx) - 1.0)


def mulaw_decode(classes, q):
    """classes of any integer value: clamped to [0, 255], then the table"""
    return mulaw_table(q)[np.clip(np.asarray(classes, dtype=np.int64), 0, 255)]


# ------------------------------------------------------------------------------------------------------------ the case grid
# (name, order, alpha, pade, scale, taps)   taps: "one" | "two" | "r64" | "r65" | "lowcut" | "r256"
CASES = [
    ("m1-p4-one", 1, 0.455, 4, 0.5, "one"),
    ("m1-p5-a0-two", 1, 0.0, 5, 0.75, "two"),
    ("m1-p4-aneg-r65", 1, -0.3, 4, 0.5, "r65"),
    ("m2-p4-lowcut", 2, 0.466, 4, 0.75, "lowcut"),
    ("m2-p5-r64", 2, 0.7, 5, 0.5, "r64"),
    ("m3-p4-r256", 3, 0.455, 4, 0.75, "r256"),
    ("m31-p5-r65", 31, 0.466, 5, 0.5, "r65"),
    ("m32-p4-lowcut", 32, 0.455, 4, 0.75, "lowcut"),
    ("m33-p5-a0-r64", 33, 0.0, 5, 0.5, "r64"),
    ("m33-p4-aneg-two", 33, -0.3, 4, 0.75, "two"),
    ("m49-p4-lowcut", 49, 0.455, 4, 0.5, "lowcut"),
    ("m49-p5-a7-r256", 49, 0.7, 5, 0.5, "r256"),
    ("m61-p4-one", 61, 0.466, 4, 0.75, "one"),
    ("m62-p5-r256", 62, 0.455, 5, 0.75, "r256"),
    ("m62-p4-aneg-lowcut", 62, -0.3, 4, 0.5, "lowcut"),
    ("m62-p5-a0-r65", 62, 0.0, 5, 0.5, "r65"),
    ("m24-p5-loud-lowcut", 24, 0.41, 5, 2.0, "lowcut"),
]
CASE_NAMES = [c[0] for c in CASES]
LENGTHS = (1, 63, 64, 65, 511, 512, 513, 1025, 1537)
N_LONG = LENGTHS[-1]
N_RESUME = 200


def low_cut_255():
    """the 255-tap 70 Hz high-pass at 22 050 Hz (tests/test_postfilter_reference.py holds dsp.low_cut_taps(22050) to it)"""
    from scipy.signal import firwin
    return firwin(255, 70.0 / (22050 // 2), pass_zero=False)


def case_taps(kind, seed):
    g = np.random.default_rng(9000 + seed)
    if kind == "one":
        return np.array([1.0])
    if kind == "two":
        return np.array([0.75, -0.25])
    if kind == "lowcut":
        return low_cut_255()
    t = g.standard_normal(int(kind[1:]))
    return t / np.abs(t).sum()


def signals(seed, n=N_LONG + N_RESUME):
    """three float32 signals: uniform(-1, 1) noise plus a 220 Hz tone, scaled into (-1, 1)"""
    g = np.random.default_rng(7000 + seed)
    t = np.arange(n)
    x = 0.45 * g.uniform(-1, 1, (3, n)) + 0.5 * np.sin(2 * np.pi * 220 * t / 22050 + np.arange(3)[:, None])
    return x.astype(np.float32)


class Case:
    """one case of the grid with what every test of it needs, computed once: coefficients, the impulse response's L1, three
    signals and their reference outputs and states after N_LONG samples, and signal 2 continued for N_RESUME samples."""

    def __init__(self, name):
        i = CASE_NAMES.index(name)
        _, self.order, self.alpha, self.pade, self.scale, self.taps_kind = CASES[i]
        self.name = name
        m = self.order
        g = np.random.default_rng(100 + i)
        mc = g.normal(size=m + 1) * self.scale / (1 + np.arange(m + 1))
        mc[0] = 0.1
        self.b = mc2b(mc, self.alpha)
        self.taps = case_taps(self.taps_kind, i)
        self.n_taps = self.taps.size
        self.seed = i
        self._cache = {}

    def _once(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    @property
    def args(self):
        return self.b, self.alpha, self.pade, self.taps

    @property
    def h(self):
        return self._once("h", lambda: impulse_response(*self.args))

    @property
    def l1(self):
        return impulse_l1(*self.args, h=self.h)[0]

    @property
    def tail(self):
        return impulse_l1(*self.args, h=self.h)[1]

    @property
    def x(self):
        return self._once("x", lambda: signals(self.seed))

    @property
    def long_run(self):
        """(y (3, N_LONG), state (3, S)) of the three signals' first N_LONG samples"""
        return self._once("long", lambda: restore_ref(self.x[:, :N_LONG], *self.args))

    @property
    def resumed(self):
        """y (N_RESUME,) of signal 2's samples N_LONG .. from the reference's own state"""
        return self._once("res", lambda: restore_ref(self.x[2, N_LONG:], *self.args, state=self.long_run[1][2])[0])

    def e64(self, xmax=1.0):
        return e64(self.order, self.pade, self.n_taps, self.l1, xmax)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]
