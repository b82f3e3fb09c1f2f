"""fp64 references, error bounds and fp32 / bf16 emulations for the per-op kernels of csrc/rg_attn.hip and csrc/rg_vae.hip.

Shared by test_attn_kernels_gpu.py, test_vae_kernels_gpu.py (kernel vs fp64 reference) and test_kernel_refs_cpu.py (emulation
vs fp64 reference: the bounds are loose enough for a correct implementation and tight enough to catch a dropped probability
column or a statistics slot of the neighbouring head group).  Every reference is torch float64 on the CPU, written from the
formulas of include/rg_gesture.h; nothing here calls the oracle's model code or a HIP kernel.

How the bounds are derived (none is read off a kernel's output)
----------------------------------------------------------------
Unit roundoffs:  U = 2^-24 (fp32 arithmetic),  US = 2^-16 (a product of a bf16 hi + lo pair with a bf16 or hi + lo operand: the
sources state ~2^-17 per product, doubled for the pair),  UB = 2^-9 (a final rounding to bf16, relative),  UE = 2^-21 (the fast
exp2-based exponentials of the MFMA self-attention modes and of the stylization's SiLU: the sources' ~1e-6, rounded up).

Dot product of n terms:  |err| <= (n U + u_product) sum_i |a_i| |b_i|, u_product = US on the matrix-core paths and 0 on the
fp32 VALU paths.  The sums of magnitudes come from the fp64 reference.

Softmax:  an absolute score error d costs a relative 2 d on each probability.  Scores that are inputs (linear attention: the
keys themselves) carry no error of their own; the subtraction of the maximum rounds with relative U, i.e. absolute
U |s - max|, which matters only where exp(s - max) does not underflow (|s - max| < 88): d <= U min(spread, 88).  The sum over
N scores adds N U, the exponential and the division a few U (fp32 paths) or UE (fast paths):
    e_P = 2 d + (N + 4) U + u_exp                                     (relative, on every probability)
Linear attention  y = Q (P^T V):  with C = sum_d |q_d| sum_n P_nd |v_nl|  (>= sum_d |q_d| |A_dl|)
    |err y| <= MARGIN ((N U + u_p + e_P) + (32 U + u_p)) C
Softmax attention  o = P V with scores s = (q scale) . k over hd terms:  d = ((hd + 1) U + u_p) max_j sum |q scale| |k_j|
    |err o| <= MARGIN (Sk U + u_p + e_P) sum_j P_j |v_j|
A bf16 output adds the final rounding, UB (|ref| + err), to the model; like every other term of the model it is multiplied by
MARGIN.  Round-to-nearest to bf16 (8 significant bits) moves a value by up to half an ulp, which is UB relative at the top of a
binade and 2 UB at its bottom, so the tests also assert the sharper form first: fp32 bound + half a bf16 ulp (`bf16_bounds`).

Statistics (sum, sum of squares over a column group) inherit the element bounds e_i:  |err sum| <= sum e_i + MARGIN n U sum |y_i|,
|err sumsq| <= sum (2 |y_i| e_i + e_i^2) + MARGIN (n + 1) U sum y_i^2.

Rounding to the 1/16 grid (masked query rows: fp32 `y + -1e6` then `+ 1e6`):  the result equals round-half-even(16 y) / 16 unless
y lies within its own error bound of a rounding tie, where one grid step is allowed (such elements are counted and printed).

LayerNorm / stylization (first-order propagation, x the fp64 row, e the element bounds of the input, sigma = sqrt(var + eps)):
    e_mu  = mean e + h U mean |x|                      h = depth of the fp32 summation (see `ln_bound`)
    two-pass variance:   e_d = e + e_mu + U |x - mu|,  e_var = 2 mean(|x - mu| e_d) + h U var
    one-pass variance (from (sum, sumsq) statistics):  e_d = e + e_mu,  e_var = 2 mean(|x| e) + h U mean x^2 + 2 |mu| e_mu
    e_xhat = (e_d + |xhat| e_var / (2 sigma)) / sigma + 4 U |xhat|        (input error over the row's standard deviation)
    e_ln   = e_xhat |gamma| + 4 U (|xhat gamma| + |beta|)                (a few U of the output magnitude)
    e_t    = e_ln |1 + scale| + 4 U (|ln (1 + scale)| + |shift|),   e_silu = 1.1 e_t + (UE + 4 U) |silu(t)|   (slope <= 1.1)
All of these are multiplied by MARGIN = 4, which covers the summation order and the dropped second-order terms.
"""
import numpy as np
import torch

U = 2.0 ** -24
US = 2.0 ** -16
UB = 2.0 ** -9
UE = 2.0 ** -21
MARGIN = 4.0
HD = 32          # head dim of the linear attention
F64 = torch.float64


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def randn(shape, seed, scale=1.0):
    return torch.from_numpy((rng(seed).standard_normal(shape) * scale).astype(np.float32))


def bf16(x):
    """Round to bf16 (nearest even), returned in x's dtype."""
    return x.float().to(torch.bfloat16).to(x.dtype)


def split_hi_lo(x):
    hi = bf16(x)
    return hi, bf16(x - hi)


def bf16_bits(x):
    """int16 bit patterns of bf16(x) -- what a kernel's bf16 output holds."""
    return x.float().to(torch.bfloat16).view(torch.int16)


def from_bf16_bits(bits):
    return bits.view(torch.bfloat16).float()


def bf16_half_ulp(x):
    """Half an ulp of bf16 (8 significant bits) at |x|: the most that round-to-nearest can move a value of that magnitude."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 8)


def bf16_bounds(ref, e):
    """Bounds for a bf16 output whose fp32 value is within e of ref (e holds the margin already): (the model with the final
    rounding, e + MARGIN UB (|ref| + e);  the sharper form: e + half an ulp of bf16 at |ref| + e)."""
    return e + MARGIN * UB * (ref.abs() + e), e + bf16_half_ulp(ref.abs() + e)


def softmax_heads(x, D):
    """The GEMM epilogue's softmax over each head's 32 columns (columns [0, D) of x)."""
    sh = x.shape
    return torch.softmax(x.double().reshape(*sh[:-1], D // HD, HD), dim=-1).reshape(sh).float()


def worst_ratio(got, ref, bound):
    """max over ALL elements of |got - ref| / bound (NaN / inf in `got` give inf)."""
    err = (got.double() - ref.double()).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = err / bound.double().clamp_min(1e-300)
    r = torch.where((err == 0), torch.zeros_like(r), r)
    return float(r.max()) if r.numel() else 0.0


# ----------------------------------------------------------------------------------------------- statistics
def group_stats(y, group):
    """(sum, sumsq) over each `group`-column part of the last dim: [..., n/group, 2]."""
    yg = y.reshape(*y.shape[:-1], y.shape[-1] // group, group)
    return torch.stack((yg.sum(-1), (yg * yg).sum(-1)), dim=-1)


def group_stats_bound(y, e, group):
    yg = y.abs().reshape(*y.shape[:-1], y.shape[-1] // group, group)
    eg = e.reshape(yg.shape)
    bs = eg.sum(-1) + MARGIN * group * U * yg.sum(-1)
    bq = (2 * yg * eg + eg * eg).sum(-1) + MARGIN * (group + 1) * U * (yg * yg).sum(-1)
    return torch.stack((bs, bq), dim=-1)


# ----------------------------------------------------------------------------------------------- linear attention
def _e_p(k, valid, N, u_exp):
    """Relative error bound of the token softmax of the keys k [R, N, H, 32] (valid [R, N] bool), per (row, head, column)."""
    kv = torch.where(valid[:, :, None, None], k, torch.full_like(k, float("nan")))
    hi = torch.nan_to_num(kv, nan=-float("inf")).max(dim=1).values
    lo = torch.nan_to_num(kv, nan=float("inf")).min(dim=1).values
    spread = (hi - lo).clamp(min=0.0, max=88.0)
    spread = torch.where(torch.isfinite(spread), spread, torch.zeros_like(spread))
    return 2 * U * spread + (N + 4) * U + u_exp          # [R, H, 32]


def sa_ref(qkv, mask, R, T, D, mfma):
    """EfficientSelfAttention core (efficient_attention.py:32-41): key + (1-mask)*-1e6, softmax over tokens, value*mask,
    A = P^T V, y = Q A.  Returns (y [R*T, D], bound [R*T, D]) in fp64; the bound is for the fp32 y."""
    H = D // HD
    x = qkv.double().view(R, T, -1)
    q, k, v = (x[..., i * D:(i + 1) * D].reshape(R, T, H, HD) for i in range(3))
    m = mask.double().view(R, T, 1, 1)
    P = torch.softmax(k + (1 - m) * -1e6, dim=1)
    A = torch.einsum("rthd,rthl->rhdl", P, v * m)
    y = torch.einsum("rthd,rhdl->rthl", q, A)
    C = torch.einsum("rthd,rhdl->rthl", q.abs(), torch.einsum("rthd,rthl->rhdl", P, (v * m).abs()))
    u_p = US if mfma else 0.0
    e_p = _e_p(k, mask.view(R, T) != 0, T, UE if mfma else 2 * U)                        # [R, H, 32(d)]
    Ce = torch.einsum("rthd,rhdl->rthl", q.abs(), torch.einsum("rthd,rthl->rhdl", P * e_p[:, None], (v * m).abs()))
    bound = MARGIN * ((T * U + u_p + HD * U + u_p) * C + Ce)
    return y.reshape(R * T, D), bound.reshape(R * T, D)


def sa_emulate(qkv, mask, R, T, D, mfma, drop=None, swap_stats=False):
    """The kernel's rounding contract in plain torch float32: masked softmax (empty set -> P = 0), then either exact fp32
    products or bf16 hi + lo operand pairs (hi*hi + hi*lo + lo*hi) with fp32 accumulation.  drop = (head, column): that
    probability column is left out (a deliberately wrong variant); swap_stats: statistics of the neighbouring head group."""
    H = D // HD
    x = qkv.float().view(R, T, -1)
    q, k, v = (x[..., i * D:(i + 1) * D].reshape(R, T, H, HD) for i in range(3))
    valid = (mask.view(R, T) != 0)[:, :, None, None]
    kk = torch.where(valid, k, torch.full_like(k, -float("inf")))
    mx = kk.max(dim=1, keepdim=True).values
    e = torch.where(valid, torch.exp(kk - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))), torch.zeros_like(k))
    s = e.sum(dim=1, keepdim=True)
    P = e * torch.where(s > 0, 1.0 / s, torch.zeros_like(s))
    if drop is not None:
        P = P.clone()
        P[:, :, drop[0], drop[1]] = 0
    if mfma:
        ph, pl = split_hi_lo(P)
        vh, vl = split_hi_lo(v)
        pv = lambda a, b: torch.einsum("rthd,rthl->rhdl", a, b)
        A = pv(pl, vh) + pv(ph, vl) + pv(ph, vh)
        ah, al = split_hi_lo(A)
        qh, ql = split_hi_lo(q)
        qa = lambda a, b: torch.einsum("rthd,rhdl->rthl", a, b)
        y = qa(ql, ah) + qa(qh, al) + qa(qh, ah)
    else:
        A = torch.einsum("rthd,rthl->rhdl", P, v)
        y = torch.einsum("rthd,rhdl->rthl", q, A)
    y = y.reshape(R * T, D)
    st = group_stats(y, 128)
    if swap_stats:
        st = st.roll(1, dims=1)
    return y, st


def grid16(y):
    """fp32 `(y + -1e6) + 1e6`: y rounded to the multiples of 1/16 (ties to even)."""
    return torch.round(y * 16) / 16


def near_tie(y, e):
    """Elements whose distance to a rounding tie of the 1/16 grid is within their own bound e."""
    f = y * 16
    return ((f - torch.floor(f) - 0.5).abs() / 16 <= e)


def ca_ref(q3, Apre, Aunc, qmask, R, Rc, T, D, ncond, u_p=0.0):
    """y3[:, c*D:(c+1)*D] = Q_c A_c (A = Apre[c][row] below Rc, Aunc[c] from Rc on), rounded to the 1/16 grid where qmask == 0.
    Returns (y [R*T, ncond*D], e [same]: element bound, tie [same] bool: masked elements that may land one grid step away)."""
    H = D // HD
    q = q3.double().view(R, T, ncond, H, HD)
    A = torch.empty(ncond, R, H, HD, HD, dtype=F64)
    if Rc > 0:
        A[:, :Rc] = Apre.double().view(ncond, Rc, H, HD, HD)
    if Rc < R:
        A[:, Rc:] = Aunc.double().view(ncond, 1, H, HD, HD)
    y = torch.einsum("rtchd,crhdl->rtchl", q, A)
    e = MARGIN * (HD * U + u_p) * torch.einsum("rtchd,crhdl->rtchl", q.abs(), A.abs())
    tie = torch.zeros_like(y, dtype=torch.bool)
    if qmask is not None:
        msk = (qmask.view(ncond, R, T) == 0).permute(1, 2, 0)[..., None, None].expand_as(y)
        tie = msk & near_tie(y, e)
        e = torch.where(msk, torch.where(tie, torch.full_like(e, 1.0 / 16), torch.zeros_like(e)), e)
        y = torch.where(msk, grid16(y), y)
    n = R * T
    return y.reshape(n, ncond * D), e.reshape(n, ncond * D), tie.reshape(n, ncond * D)


def ca_emulate(q3, Apre, Aunc, qmask, R, Rc, T, D, ncond):
    H = D // HD
    q = q3.float().view(R, T, ncond, H, HD)
    A = torch.empty(ncond, R, H, HD, HD)
    if Rc > 0:
        A[:, :Rc] = Apre.view(ncond, Rc, H, HD, HD)
    if Rc < R:
        A[:, Rc:] = Aunc.view(ncond, 1, H, HD, HD)
    y = torch.einsum("rtchd,crhdl->rtchl", q, A)
    if qmask is not None:
        msk = (qmask.view(ncond, R, T) == 0).permute(1, 2, 0)[..., None, None].expand_as(y)
        z = y + torch.tensor(-1000000.0)
        y = torch.where(msk, z + torch.tensor(1000000.0), y)
    return y.reshape(R * T, ncond * D)


def kv_reduce_ref(kv, B, N, D):
    """A[b][h] = softmax_N(K)^T V (efficient_attention.py:82-90); returns (A [B, H, 32, 32], bound)."""
    H = D // HD
    x = kv.double().view(B, N, -1)
    k, v = x[..., :D].reshape(B, N, H, HD), x[..., D:2 * D].reshape(B, N, H, HD)
    P = torch.softmax(k, dim=1)
    A = torch.einsum("bnhd,bnhl->bhdl", P, v)
    e_p = _e_p(k, torch.ones(B, N, dtype=torch.bool), N, 2 * U)
    bound = MARGIN * (N * U + e_p)[..., None] * torch.einsum("bnhd,bnhl->bhdl", P, v.abs())
    return A, bound


def kv_reduce_emulate(kv, B, N, D):
    H = D // HD
    x = kv.float().view(B, N, -1)
    k, v = x[..., :D].reshape(B, N, H, HD), x[..., D:2 * D].reshape(B, N, H, HD)
    e = torch.exp(k - k.max(dim=1, keepdim=True).values)
    return torch.einsum("bnhd,bnhl->bhdl", e / e.sum(dim=1, keepdim=True), v)


# ----------------------------------------------------------------------------------------------- LayerNorm / stylization
def ln_bound(x, e, gamma, beta, eps, depth, one_pass):
    """fp64 LayerNorm of the rows x [rows, n] with the element bounds e of the input; returns (ln, e_ln) -- e_ln WITHOUT the
    margin.  depth: depth of the fp32 summations in units of U (a wave sums n/64 elements per lane and then 6 butterfly steps:
    n/64 + 6; statistics that arrive as partial sums: additions per partial + number of partials)."""
    n = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    sigma = torch.sqrt(var + eps)
    xh = d / sigma
    e = e if torch.is_tensor(e) else torch.full_like(x, float(e))
    e_mu = e.mean(-1, keepdim=True) + depth * U * x.abs().mean(-1, keepdim=True)
    if one_pass:
        e_d = e + e_mu
        e_var = 2 * (x.abs() * e).mean(-1, keepdim=True) + depth * U * (x * x).mean(-1, keepdim=True) + 2 * mu.abs() * e_mu
    else:
        e_d = e + e_mu + U * d.abs()
        e_var = 2 * (d.abs() * e_d).mean(-1, keepdim=True) + depth * U * var
    e_xh = (e_d + xh.abs() * e_var / (2 * sigma)) / sigma + 4 * U * xh.abs()
    ln = xh * gamma + beta
    return ln, e_xh * gamma.abs() + 4 * U * ((xh * gamma).abs() + beta.abs())


def styl_ref(x, e, gamma, beta, scale, shift, depth, eps=1e-5):
    """StylizationBlock front half (stylization_block.py:36-39): SiLU(LN(x) * (1 + scale) + shift) from one-pass statistics.
    e: element bounds of x WITHOUT the margin.  Returns (out fp64, bound of the fp32 value with the margin); a bf16 output goes
    through `bf16_bounds`.  scale = shift = None: the LayerNorm alone."""
    ln, e_ln = ln_bound(x, e, gamma, beta, eps, depth, True)
    if scale is None:
        return ln, MARGIN * e_ln
    t = ln * (1 + scale) + shift
    e_t = e_ln * (1 + scale).abs() + 4 * U * ((ln * (1 + scale)).abs() + shift.abs())
    out = t * torch.sigmoid(t)
    return out, MARGIN * (1.1 * e_t + (UE + 4 * U) * out.abs())


def styl_emulate(x, stats, gamma, beta, scale, shift, eps=1e-5):
    """fp32 emulation of the stylization from partial (sum, sumsq) statistics [rows, nparts, 2], rounded to bf16 at the end."""
    x, n = x.float(), x.shape[-1]
    mu = stats[..., 0].float().sum(-1, keepdim=True) / n
    var = (stats[..., 1].float().sum(-1, keepdim=True) / n - mu * mu).clamp_min(0.0)
    t = (x - mu) * torch.rsqrt(var + eps) * gamma + beta
    if scale is not None:
        t = t * (1.0 + scale) + shift
        t = t * torch.sigmoid(t)
    return bf16(t)


def split_transpose_ref(A):
    """At[m] = (bf16(A[m]^T), bf16(A[m]^T - hi)) as int16 bit patterns [n, 2, 32, 32] (rg_split_transpose_bf16)."""
    At = A.float().transpose(-1, -2).contiguous()
    hi = At.to(torch.bfloat16)
    lo = (At - hi.float()).to(torch.bfloat16)
    return torch.stack((hi.view(torch.int16), lo.view(torch.int16)), dim=-3).contiguous()


def ca_stylize_ref(q3, A, qmask, gamma, beta, ss_rows, Rc, T, D, ncond):
    """rg_ca_stylize on the conditional rows: y = Q A (bf16 hi + lo pairs: u_p = US), the 1/16 grid where qmask == 0, LayerNorm
    over D from one-pass statistics (32 columns per wave in two chains, then 16 waves: depth 34), * (1 + scale) + shift, SiLU.
    ss_rows [Rc, ncond, 2 D]: the (scale | shift) of each row group.  Returns (out [Rc*T, ncond*D], bound of the fp32 value,
    number of masked elements within their bound of a rounding tie)."""
    y, e, tie = ca_ref(q3, A, None, qmask, Rc, Rc, T, D, ncond, u_p=US)
    y, e = y.view(Rc, T, ncond, D), e.view(Rc, T, ncond, D) / MARGIN
    g, b = gamma.double().view(1, 1, ncond, D), beta.double().view(1, 1, ncond, D)
    ss = ss_rows.double().view(Rc, 1, ncond, 2 * D)
    out, err = styl_ref(y, e, g, b, ss[..., :D], ss[..., D:], 34)
    return out.reshape(Rc * T, ncond * D), err.reshape(Rc * T, ncond * D), int(tie.sum())


def layernorm_ref(x, res, gamma, beta, eps):
    """nn.LayerNorm of fp32 rows (+ residual), two-pass; returns (out fp64, bound for the fp32 output)."""
    xd = x.double() + (res.double() if res is not None else 0.0)
    e = U * xd.abs() if res is not None else 0.0          # the fp32 x + residual
    ln, e_ln = ln_bound(xd, e, gamma.double(), beta.double(), eps, (x.shape[-1] + 63) // 64 + 6, False)
    return ln, MARGIN * e_ln


def layernorm_emulate(x, res, gamma, beta, eps, one_pass=False):
    x = x.float() + (res.float() if res is not None else 0.0)
    mean = x.sum(-1, keepdim=True) / x.shape[-1]
    if one_pass:      # a deliberately fragile variant: E[x^2] - mean^2 in fp32
        var = (x * x).sum(-1, keepdim=True) / x.shape[-1] - mean * mean
    else:
        d = x - mean
        var = (d * d).sum(-1, keepdim=True) / x.shape[-1]
    return (x - mean) * torch.rsqrt(var + eps) * gamma + beta


# ----------------------------------------------------------------------------------------------- softmax attention
def mha_ref(q, k, v, B, H, Sq, Sk, hd, mfma):
    """softmax(Q K^T / sqrt(hd)) V per (batch, head) (nn.MultiheadAttention core).  q [B*Sq, >= H*hd], k / v [B*Sk, >= H*hd]
    (column slices are fine).  mfma: K and V are rounded to bf16 first (the kernel's contract), Q is not.
    Returns (o [B*Sq, H*hd] fp64, bound for the fp32 output)."""
    qd = q[:, :H * hd].double().reshape(B, Sq, H, hd)
    kd = (bf16(k[:, :H * hd]) if mfma else k[:, :H * hd]).double().reshape(B, Sk, H, hd)
    vd = (bf16(v[:, :H * hd]) if mfma else v[:, :H * hd]).double().reshape(B, Sk, H, hd)
    sc = 1.0 / float(hd) ** 0.5
    s = torch.einsum("bihd,bjhd->bhij", qd * sc, kd)
    P = torch.softmax(s, dim=-1)
    o = torch.einsum("bhij,bjhd->bihd", P, vd)
    u_p = US if mfma else 0.0
    d = ((hd + 1) * U + u_p) * torch.einsum("bihd,bjhd->bhij", (qd * sc).abs(), kd.abs()).max(dim=-1).values      # [B, H, Sq]
    spread = (s.max(dim=-1).values - s.min(dim=-1).values).clamp(max=88.0)
    e_p = 2 * (d + U * spread) + (Sk + 4) * U + 2 * U
    bound = MARGIN * (Sk * U + u_p + e_p).permute(0, 2, 1)[..., None] * torch.einsum("bhij,bjhd->bihd", P, vd.abs())
    return o.reshape(B * Sq, H * hd), bound.reshape(B * Sq, H * hd)


def mha_emulate(q, k, v, B, H, Sq, Sk, hd, mfma, drop_key=None):
    """fp32 emulation: (mfma) K, V rounded to bf16, Q * scale and P as bf16 hi + lo pairs, fp32 accumulation.  drop_key: that
    key's probability is left out of P V (a deliberately wrong variant)."""
    qf = q[:, :H * hd].float().reshape(B, Sq, H, hd) * torch.tensor(1.0 / float(hd) ** 0.5, dtype=torch.float32)
    kf, vf = k[:, :H * hd].float().reshape(B, Sk, H, hd), v[:, :H * hd].float().reshape(B, Sk, H, hd)
    if mfma:
        kf, vf = bf16(kf), bf16(vf)
        qh, ql = split_hi_lo(qf)
        s = torch.einsum("bihd,bjhd->bhij", qh, kf) + torch.einsum("bihd,bjhd->bhij", ql, kf)
    else:
        s = torch.einsum("bihd,bjhd->bhij", qf, kf)
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    P = e * (1.0 / e.sum(dim=-1, keepdim=True))
    if drop_key is not None:
        P = P.clone()
        P[..., drop_key] = 0
    if mfma:
        ph, pl = split_hi_lo(P)
        o = torch.einsum("bhij,bjhd->bihd", ph, vf) + torch.einsum("bhij,bjhd->bihd", pl, vf)
    else:
        o = torch.einsum("bhij,bjhd->bihd", P, vf)
    return o.reshape(B * Sq, H * hd)


# ----------------------------------------------------------------------------------------------- canaries
def canary(rows, cols, dtype=torch.float32, value=None):
    """A CPU buffer filled with a sentinel (NaN by default for float buffers; bf16 buffers are int16 bit patterns)."""
    if dtype == torch.int16:
        return torch.full((rows, cols), 0x7FC1 if value is None else value, dtype=torch.int16)
    return torch.full((rows, cols), float("nan") if value is None else value, dtype=dtype)


def untouched(got, before, rows, c0, c1):
    """True when `got` equals `before` bit for bit outside rows [0, rows) x columns [c0, c1)."""
    a, b = got.cpu().contiguous(), before.contiguous()
    ai = a.view(torch.int32 if a.element_size() == 4 else torch.int16).clone()
    bi = b.view(torch.int32 if b.element_size() == 4 else torch.int16).clone()
    ai[:rows, c0:c1] = 0
    bi[:rows, c0:c1] = 0
    return bool(torch.equal(ai, bi))
