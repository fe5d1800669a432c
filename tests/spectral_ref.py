"""A float64 reference of the multi-resolution STFT loss (csrc/swn_spectral.hip) for the tests: plain torch on the CPU.

What the GPU tests compare with, and why it is built this way (test_spectral_reference.py checks each claim on the CPU):

* The operator transforms d = sample - target, stores the sign of every coefficient of STFT(d) as its state and, in the
  backward, multiplies those signs with the basis.  With the signs held fixed the backward is the gradient of a LINEAR
  function of the samples, sum_rk g[r, k] / count_k * sum(s_re * Re STFT(x) + s_im * Im STFT(x)): `grad_from_signs` takes
  it from torch.stft + autograd, no hand-written overlap-add.
* The structural set (`structural_mask`): with reflect padding a frame centred on sample 0 or on sample T - 1 is symmetric
  about its centre, so every imaginary part of it is zero in exact arithmetic, and so are the imaginary parts of bin 0 and
  bin n / 2 of every frame.  In floating point those entries are rounding noise of random sign; the fold of the backward
  cancels what they contribute (to 1e-16 of the gradient), so they are not compared and are zero in the reference.
* `worst_case_bound`: no fp32 evaluation of a coefficient, in any order, moves it further than (n + 3) * 2^-24 times the
  sum of |d| * window over the frame (n terms, whose factors carry three roundings: table entry, window, their product).
  A coefficient larger than that has the same sign in fp32 as in float64; only the ones below it are left out of the sign
  comparison, and the tests cap their share at 1 %.
"""
import numpy as np
import torch

FFT17 = [128, 160, 192, 224, 256, 320, 384, 448, 512, 640, 768, 896, 1024, 1280, 1536, 1792, 2048]
EDGE_SIZES = [32, 96, 160, 1024, 2016, 2048]
BELOW_BOUND_CAP = 0.01         # share of the non-structural entries of a case that may lie below worst_case_bound


def frames_of(T, n):
    return 1 + T // (n // 4)


def bins_of(n):
    return n // 2 + 1


def signals(R, length, seed):
    """targets: smoothed noise through tanh; samples: targets + 0.02 N(0, 1), clamped to [-1, 1] (float64, CPU).
    The smoothing is a one-pole low-pass (0.6^k, 16 taps: -12 dB at the Nyquist frequency, no spectral null), so that every
    bin of the target holds power well above fp32 rounding and the LSD figure is as well conditioned as on speech: with a
    kernel that has nulls torch's own fp32 path returns inf for some (row, size) where float64 is finite, and a bound
    derived from it says nothing."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(R, 1, length + 15, generator=g, dtype=torch.float64)
    kernel = (0.6 ** torch.arange(16, dtype=torch.float64)).flip(0).view(1, 1, -1)
    trg = torch.tanh(torch.nn.functional.conv1d(noise, kernel)[:, 0, :length] * 0.4)
    smp = (trg + 0.02 * torch.randn(R, length, generator=g, dtype=torch.float64)).clamp(-1.0, 1.0)
    return smp, trg


def signals_f32(R, length, seed):
    """`signals` rounded to fp32 (what the operator is given), as float64 tensors: smp, trg, d = smp - trg (exact)"""
    smp, trg = signals(R, length, seed)
    smp, trg = smp.float().double(), trg.float().double()
    return smp, trg, smp - trg


def silence(trg, start=3001, width=700):
    """`width` consecutive exact zeros in every target row"""
    trg = trg.clone()
    trg[:, start:start + width] = 0.0
    return trg


def stft(x, n, dtype=torch.float64):
    """torch.stft with its defaults (hop n / 4, reflect-centred, one-sided) and the periodic Hann window, in `dtype`, as
    reals: (R, bins, frames, 2)"""
    return torch.view_as_real(torch.stft(x.to(dtype), n, window=torch.hann_window(n, dtype=dtype), return_complex=True))


def stft64(x, n):
    return stft(x, n, torch.float64)


def structural_mask(n, T, bins, frames):
    """bool (bins, frames, 2): the entries that are zero in exact arithmetic whatever the signal: Im of bins 0 and n / 2,
    and Im of every bin of a frame centred on sample 0 or on sample T - 1"""
    assert bins == bins_of(n) and frames == frames_of(T, n)
    hop = n // 4
    m = torch.zeros(bins, frames, 2, dtype=torch.bool)
    m[0, :, 1] = True
    m[n // 2, :, 1] = True
    for f in range(frames):
        if f * hop == 0 or f * hop == T - 1:
            m[:, f, 1] = True
    return m


def worst_case_bound(d, n):
    """(R, frames) float64: (n + 3) * 2^-24 * sum_j |d_pad[f * hop + j]| * w[j], for every bin of that frame"""
    d = d.double()
    pad = torch.nn.functional.pad(d.abs().unsqueeze(1), (n // 2, n // 2), mode="reflect")[:, 0]
    fr = pad.unfold(1, n, n // 4)                                       # (R, frames, n)
    assert fr.shape[1] == frames_of(d.shape[1], n)
    return (n + 3) * 2.0 ** -24 * (fr * torch.hann_window(n, dtype=torch.float64)).sum(-1)


def decode_state(state, R, T, sizes):
    """the operator's byte state -> per size an int8 tensor (R, bins, frames, 2) in {-1, 0, +1}.  Layout (include/swn_hip.h):
    the sizes in call order, per size [row][frame][bin]; bits 0-1 the real part, bits 2-3 the imaginary part, 1 = positive,
    2 = negative, 0 = zero; nothing else may be set."""
    state = torch.as_tensor(state).cpu().reshape(-1)
    assert state.dtype == torch.uint8
    assert state.numel() == sum(R * frames_of(T, n) * bins_of(n) for n in sizes), "state size"
    lut = torch.tensor([0, 1, -1, 99], dtype=torch.int8)
    out, at = [], 0
    for n in sizes:
        fr, bn = frames_of(T, n), bins_of(n)
        s = state[at:at + R * fr * bn].reshape(R, fr, bn).long()
        at += R * fr * bn
        assert int((s >> 4).max()) == 0, f"size {n}: bits 4-7 set"
        v = torch.stack([lut[s & 3], lut[(s >> 2) & 3]], -1).permute(0, 2, 1, 3).contiguous()
        assert int(v.max()) <= 1, f"size {n}: sign code 3"
        out.append(v)
    return out


def grad_from_signs(x, signs, sizes, g, dtype=torch.float64):
    """gradient in x (R, T) of sum_k sum_r g[r, k] / count_k * sum(signs_k[r] * STFT_k(x)[r]) evaluated in `dtype`, count_k =
    bins * frames * 2: what the operator's backward computes from the state `signs` (linear in x: the values of x do not
    enter).  Returned in float64."""
    x = x.to(dtype).clone().requires_grad_(True)
    g = g.to(dtype)
    total = x.new_zeros(())
    for k, (n, s) in enumerate(zip(sizes, signs)):
        sp = stft(x, n, dtype)
        total = total + ((s.to(dtype) * sp).sum(dim=(1, 2, 3)) * g[:, k]).sum() / (sp.shape[1] * sp.shape[2] * 2)
    total.backward()
    return x.grad.double()


def grad64_from_signs(x, signs, sizes, g):
    return grad_from_signs(x, signs, sizes, g, torch.float64)


def terms(smp, trg, sizes, dtype):
    """`batch_loss`'s torch formulas per (row, size) on the CPU in `dtype`: l1 (R, K) and lsd (R, K), attached to `smp`"""
    R = smp.shape[0]
    l1, lsd = [], []
    for n in sizes:
        sp = stft(torch.cat([smp, trg.to(dtype)]), n, dtype)
        so, st = sp[:R], sp[R:]
        l1.append(torch.abs(so - st).mean(dim=(1, 2, 3)))
        px, py = torch.sum(so ** 2, -1), torch.sum(st ** 2, -1)
        lsd.append(torch.sqrt(torch.mean((10 * (torch.log10(px) - torch.log10(py))) ** 2, 1)).mean(1))
    return torch.stack(l1, 1), torch.stack(lsd, 1)


def torch_path(smp, trg, sizes, dtype):
    """-> l1 (R, K), lsd (R, K), d mean(l1) / d smp of the torch formulas in `dtype`, returned in float64"""
    smp = smp.to(dtype).clone().requires_grad_(True)
    l1, lsd = terms(smp, trg, sizes, dtype)
    l1.mean().backward()
    return l1.detach().double(), lsd.detach().double(), smp.grad.double()


def loss64(smp, trg, sizes):
    """l1 and lsd per (row, size) in float64"""
    with torch.no_grad():
        l1, lsd = terms(smp.double(), trg, sizes, torch.float64)
    return l1, lsd


def true_grad64(smp, trg, sizes, g):
    """d sum(g * l1) / d smp by autograd of the |.| loss itself, float64"""
    smp = smp.double().clone().requires_grad_(True)
    l1, _ = terms(smp, trg, sizes, torch.float64)
    (l1 * g.double()).sum().backward()
    return smp.grad


def weights(R, K, seed):
    """the upstream gradient of the tests: (R, K) float32 values in [-1, 1] with exact zeros, negative entries and, for
    R > 1, one all-zero row (row R // 2).  Row 0 keeps every entry, its first one negative."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.rand(R, K, generator=gen) * 2 - 1
    drop = torch.rand(R, K, generator=gen) < 0.15
    drop[0] = False
    g[drop] = 0.0
    g[0, 0] = -0.25 - 0.75 * g[0, 0].abs()
    if R > 1:
        g[R // 2] = 0.0
    return g


def sign_report(d, n, signs):
    """signs (R, bins, frames, 2) of some evaluation of STFT_n(d) against float64.  Returns a dict: `compared` entries
    (outside the structural set, above the bound), `left_out` (outside, below the bound), `nonstructural`, `structural`,
    and how many of each differ from the float64 sign: `bad`, `left_out_diff`, `structural_diff`; plus the tensors
    `ref` (float64 signs, structural set zeroed), `below` (bool, the left-out entries) for building the gradient reference."""
    R, T = d.shape
    c = stft64(d, n)
    ref = torch.sign(c).to(torch.int8)
    st = structural_mask(n, T, c.shape[1], c.shape[2]).expand_as(c)
    above = c.abs() > worst_case_bound(d, n)[:, None, :, None]
    diff = torch.as_tensor(signs).to(torch.int8) != ref
    below = ~st & ~above
    ref = torch.where(st, torch.zeros_like(ref), ref)
    return dict(compared=int((~st & above).sum()), left_out=int(below.sum()), nonstructural=int((~st).sum()),
                structural=int(st.sum()), bad=int((diff & ~st & above).sum()), left_out_diff=int((diff & below).sum()),
                structural_diff=int((diff & st).sum()), ref=ref, below=below)


def shuffled(sizes, seed):
    p = np.random.Generator(np.random.PCG64(seed)).permutation(len(sizes))
    return [sizes[i] for i in p]


def cases():
    """the table of the GPU tests: (id, rows, length, sizes, seed)"""
    out = [("recipe-5x8114", 5, 8114, FFT17, 8114),
           ("sizes-32-1024", 2, 1100, list(range(32, 1025, 32)), 1100),
           ("sizes-1056-2048", 2, 1100, list(range(1056, 2049, 32)), 1100),
           ("single-2048", 3, 4999, [2048], 4999),
           ("single-32", 3, 4999, [32], 4999),
           ("order-descending", 2, 1100, FFT17[::-1], 1101),
           ("order-shuffled", 2, 1100, shuffled(FFT17, 17), 1101),
           ("order-512-128-512", 2, 1100, [512, 128, 512], 1101)]
    for n in EDGE_SIZES:
        for T in (n // 2 + 1, n // 2 + 2):
            out.append((f"short-n{n}-T{T}", 4, T, [n], 7 * n + T))
    for n in EDGE_SIZES:
        hop = n // 4
        for T in (7 * hop - 1, 7 * hop, 8 * hop, 15 * hop, 16 * hop, 16 * hop + 1):
            out.append((f"tile-n{n}-T{T}", 4, T, [n], 7 * n + T))
    out += [("rows-16x2500", 16, 2500, [n for n in FFT17 if 2500 > n // 2], 2500),
            ("rows-10x8114", 10, 8114, FFT17, 8115)]
    return out


def rel(a, ref, mask=None):
    if mask is not None:
        a, ref = a[mask], ref[mask]
    return float((a - ref).abs().max() / ref.abs().max())
