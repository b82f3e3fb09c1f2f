"""fp64 references, error bounds and fp32 / bf16 emulations for the per-op kernels of csrc/rg_attn.hip and csrc/rg_vae.hip and
for the fused GEMM family (csrc/rg_gemm*.hip, rg_gemm_epi.h).

Shared by test_attn_kernels_gpu.py, test_vae_kernels_gpu.py, test_gemm_kernels_gpu.py (kernel vs fp64 reference) and test_kernel_refs_cpu.py (emulation
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

Fused GEMM (rg_gemm: `gemm_ref`, `gemm_emulate`)
-------------------------------------------------
out[M, N] = epilogue(A'[M, K] W[N, K]^T) (include/rg_gesture.h: rg_gemm_desc).  The matrix cores multiply bf16 operands
exactly and accumulate in fp32, so the only error of the product is the accumulation: n U sum |a| |w|.

Operand tiers (E_A is the per-element distance between the kernel's operand and the reference's, 0 where they agree):
  exact      identity fp32 segments, bf16 A: the reference rounds A to bf16 (nearest even) itself; E_A = 0.
  W_lo       hi + lo planes of A and W, hi lo + lo hi + hi hi: the reference takes the fp32 A and W = hi + lo; the dropped
             lo lo term and the rounding of the lo planes are the US of the file: u_p = US, E_A = e_k (prologue) or 0.
  prologue   LN / STYL segments and the stylized bf16 A: the kernel rounds an fp32 x~ with |x~ - x| <= e_k (`styl_ref`, one-pass
             statistics summed from nparts fp32 partials: depth nparts + 1) to bf16: E_A = e_k + half a bf16 ulp at |x| + e_k.
  e_acc = MARGIN (K U + u_p) sum_k |a_k| |w_k| + sum_k E_A,k |w_k|
Folded LayerNorm  out = rstd (acc - mean c1):  mean and variance come from one-pass partials of the fp32 rows (e_mu, e_var
as in `ln_bound`, depth ln_nparts + 1), e_rstd = rstd e_var / (2 (var + eps)), and the fp32 product mean * c1 and the
difference round with U of |mean c1| -- the cancellation term, proportional to |mean| |c1| and not to the small result:
  e = rstd e_acc + MARGIN (e_rstd |acc - mean c1| + rstd (e_mu |c1| + 2 U |mean c1| + U |acc - mean c1|) + U |out|)
Every fp32 elementwise step (bias, tbias, residual) adds MARGIN U |result|.
Softmax over 32 columns: scores with absolute errors e_j give every probability the relative error 2 max_j e_j (its own
score and the normaliser), then the file's e_P with N = 32: + MARGIN (2 U min(spread, 88) + 36 U + u_exp), u_exp = UE
(__expf) for bf16-operand GEMMs and 4 U (libm expf) in W_lo mode.
GELU(v) = v/2 (1 + erf(v / sqrt 2)), slope <= 1.13:  e' = 1.13 e + MARGIN (|v|/2 e_erf + 2 U |gelu|); the fast path computes
erf by Abramowitz-Stegun 7.1.26, whose published absolute error is 1.5e-7 (GELU_AS), on the fast reciprocal and exp2 (UE):
e_erf = GELU_AS + UE; libm erff (W_lo mode): e_erf = 4 U.  The error of erf is absolute, so the bound is proportional to
|v| and not to the (possibly tiny, v << 0) result.  ReLU does not change e.
Statistics: `group_stats_bound` per column tile over the final fp32 values (columns past N count as 0); bf16 outputs:
`bf16_bounds`.
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


# ----------------------------------------------------------------------------------------------- fused GEMM (rg_gemm)
# (derivation of the bounds: module docstring, "Fused GEMM")
GELU_AS = 1.5e-7
GEMM_MUTANTS = ("trunc_a", "drop_k_tail", "tbias_row", "res_ldo", "stats_slot", "softmax_shift", "ln_kpad", "styl_noscale",
                "gb_group0", "wlo_no_hilo")


class GemmCase:
    """One rg_gemm problem on CPU tensors, filled by `gemm_case` only.  Fields:
    every case    name, variant, path, waves; M, N, K; kind ("f32" / "bf16" / "styl"); w [N, K]; wlo; a_row_mod; groups, gb_group,
                  gb_stride; bias [N] / None; tb, tbias [tb, N] / None; softmax_cols; act; res [M, ldr] / None, ldr; out_bf16, ldo,
                  out_off; want_stats; want_out2, ldo2; split_col; tile_n; ln (partials of the folded LayerNorm, 0 = none)
    kind "f32"    src [rows, ld], ld; nseg, seg_len, modes, col (first column of each segment); nparts; per segment (None for
                  IDENT): stats [rows, nparts, 2], gamma / beta [groups or 1, seg_len], ss [2 seg_len] (STYL)
    bf16 / styl   x [rows, lda] (the fp32 rows), a = bf16(x), lda; styl: nparts, st [rows, nparts, 2], gain, offset [K]
    ln > 0        ln_stats [M, ln, 2], c1 [N]"""


def _partials(x, nparts):
    """[rows, nparts, 2] fp32 (sum, sumsq) over nparts column chunks (as equal as possible) of the fp64 rows x."""
    ch = torch.tensor_split(x.double(), nparts, dim=-1)
    return torch.stack([torch.stack((c.sum(-1), (c * c).sum(-1)), -1) for c in ch], dim=-2).float().contiguous()


def gemm_case(name, M, N, K, seed, *, kind="f32", modes=None, seg_len=None, nparts=4, ld_pad=0, col0=0, a_row_mod=0, groups=0,
              wlo=False, bias=True, tb=0, softmax_cols=0, act=0, res=False, ldr_pad=0, out_bf16=False, ldo_pad=8, out_off=0,
              stats=False, out2=False, ldo2_pad=8, split_col=0, ln=0, tile_n=0, path=0, waves=0, variant=""):
    """Inputs of one case, all on the CPU.  kind: "f32" (segments of `modes`, a list of 0 IDENT / 1 LN / 2 STYL; one source
    tensor [rows, col0 + nseg seg_len + ld_pad], segment s at column col0 + s seg_len), "bf16", "styl" (stylized bf16 A).
    groups > 0: gb_group = N / groups, every group with its own gamma / beta (fp32) or its own K columns of A (bf16).
    ln: partials of the folded LayerNorm (0 = none).  *_pad: extra columns of the leading dimension; out_off: element offset
    of `out` inside its buffer.  path / waves: the selection hooks; variant: the instantiation the dispatch code reaches."""
    c = GemmCase()
    c.name, c.M, c.N, c.K, c.kind, c.path, c.waves, c.variant = name, M, N, K, kind, path, waves, variant
    c.a_row_mod, c.groups, c.wlo, c.tb, c.softmax_cols, c.act = a_row_mod, groups, wlo, tb, softmax_cols, act
    c.out_bf16, c.ldo, c.out_off, c.want_stats, c.want_out2, c.split_col = out_bf16, N + ldo_pad, out_off, stats, out2, split_col
    c.ldo2, c.ln, c.tile_n = (N - split_col) + ldo2_pad, ln, tile_n
    c.gb_group = N // groups if groups else 0
    rows = a_row_mod if a_row_mod else M
    s = iter(range(seed * 100, seed * 100 + 100))
    c.w = randn((N, K), next(s), 0.05)
    ng = max(groups, 1)
    if kind == "f32":
        c.modes = list(modes or [0])
        c.nseg = len(c.modes)
        c.seg_len = seg_len if seg_len is not None else ((K + 63) // 64 * 64 if c.nseg == 1 else 512)
        width = c.seg_len if c.nseg > 1 else max(K, c.seg_len if any(c.modes) else K)
        c.ld = col0 + (c.nseg - 1) * c.seg_len + width + ld_pad
        c.src = randn((rows, c.ld), next(s), 1.3) + 0.4
        c.col = [col0 + i * c.seg_len for i in range(c.nseg)]
        c.nparts, c.gb_stride = nparts, c.seg_len
        c.stats = [_partials(c.src[:, c.col[i]:c.col[i] + c.seg_len], nparts) if m else None for i, m in enumerate(c.modes)]
        c.gamma = [1 + 0.2 * randn((ng, c.seg_len), next(s)) if m else None for m in c.modes]
        c.beta = [0.2 * randn((ng, c.seg_len), next(s)) if m else None for m in c.modes]
        c.ss = [randn((2 * c.seg_len,), next(s), 0.3) if m == 2 else None for m in c.modes]
    else:
        c.gb_stride = K
        c.lda = ng * K + (ld_pad or 8)
        c.x = randn((rows, c.lda), next(s), 1.3) + 0.4          # the fp32 rows; A is their bf16 copy
        if kind == "styl":
            c.x = bf16(c.x)                                      # the block output is taken as bf16-exact: one LayerNorm to model
            c.nparts = nparts
            c.st = _partials(c.x[:, :K], nparts)
            g, b, ss = 1 + 0.2 * randn((K,), next(s)), 0.2 * randn((K,), next(s)), randn((2 * K,), next(s), 0.3)
            c.gain, c.offset = (g * (1 + ss[:K])).contiguous(), (b * (1 + ss[:K]) + ss[K:]).contiguous()
        c.a = bf16(c.x)
    if ln:
        c.ln_stats = _partials(c.x[:, :K], ln)
        c.c1 = bf16(c.w).double().sum(-1).float()
    c.bias = randn((N,), next(s)) if bias else None
    c.tbias = randn((tb, N), next(s)) if tb else None
    c.ldr = N + ldr_pad
    c.res = randn((M, c.ldr), next(s)) if res else None
    return c


def _gelu64(v):
    return 0.5 * v * (1 + torch.erf(v * 0.7071067811865476))


def _gemm_operand(c, g):
    """fp64 operand [M, K] of column group g and its distance bound E_A (None where the operand is exact)."""
    K = c.K
    rmap = torch.arange(c.M) % c.a_row_mod if c.a_row_mod else torch.arange(c.M)
    if c.kind == "bf16":
        return c.a[:, g * c.gb_stride:g * c.gb_stride + K].double()[rmap], None
    if c.kind == "styl":
        x, e = styl_ref(c.a[:, :K].double(), 0.0, c.gain.double(), c.offset.double(), torch.zeros(K, dtype=F64),
                        torch.zeros(K, dtype=F64), c.nparts + 1)
        return x[rmap], (e + bf16_half_ulp(x.abs() + e))[rmap]
    cols, errs = [], []
    for i, m in enumerate(c.modes):
        n = min(c.seg_len, K - i * c.seg_len)
        x = c.src[:, c.col[i]:c.col[i] + (c.seg_len if m else n)].double()
        if m == 0:
            cols.append(x if c.wlo else bf16(x))
            errs.append(torch.zeros_like(x))
            continue
        ga, be = c.gamma[i][g].double(), c.beta[i][g].double()
        sc, sh = (c.ss[i][:c.seg_len].double(), c.ss[i][c.seg_len:].double()) if m == 2 else (None, None)
        y, e = styl_ref(x, 0.0, ga, be, sc, sh, c.nparts + 1)
        cols.append(y[:, :n])
        errs.append((e if c.wlo else e + bf16_half_ulp(y.abs() + e))[:, :n])
    return torch.cat(cols, -1)[rmap], (torch.cat(errs, -1)[rmap] if any(c.modes) else None)


def gemm_ref(c):
    """fp64 reference of case c.  Returns a dict: out [M, n_out] and its bound e (fp32 value; bf16 outputs go through
    `bf16_bounds`), n_out = split_col or N;  stats / e_stats [M, tiles, 2] (want_stats);  out2 / e2 [M, N - split_col]: the
    fp32 value whose bf16 rounding out2 holds (want_out2)."""
    M, N, K = c.M, c.N, c.K
    w = (bf16(c.w) + bf16(c.w - bf16(c.w)) if c.wlo else bf16(c.w)).double()
    u_p = US if c.wlo else 0.0
    ng = max(c.groups, 1)
    gw = N // ng
    acc, e = torch.empty(M, N, dtype=F64), torch.empty(M, N, dtype=F64)
    for g in range(ng):
        a, ea = _gemm_operand(c, g)
        wg = w[g * gw:(g + 1) * gw]
        acc[:, g * gw:(g + 1) * gw] = a @ wg.T
        e[:, g * gw:(g + 1) * gw] = MARGIN * (K * U + u_p) * (a.abs() @ wg.abs().T) + (ea @ wg.abs().T if ea is not None else 0.0)
    v = acc
    if c.ln:
        x = c.x[:, :K].double()
        mu, msq = x.mean(-1, keepdim=True), (x * x).mean(-1, keepdim=True)
        var = msq - mu * mu
        rs = torch.rsqrt(var + 1e-5)
        depth = c.ln + 1
        e_mu = depth * U * x.abs().mean(-1, keepdim=True)
        e_var = depth * U * msq + 2 * mu.abs() * e_mu
        e_rs = rs * e_var / (2 * (var + 1e-5))
        c1 = c.c1.double()[None, :]
        dif = acc - mu * c1
        v = rs * dif
        e = rs * e + MARGIN * (e_rs * dif.abs() + rs * (e_mu * c1.abs() + 2 * U * (mu * c1).abs() + U * dif.abs()) + U * v.abs())
    if c.bias is not None:
        v = v + c.bias.double()[None, :]
        e = e + MARGIN * U * v.abs()
    if c.tb:
        v = v + c.tbias.double()[torch.arange(M) % c.tb]
        e = e + MARGIN * U * v.abs()
    if c.softmax_cols:
        D = c.softmax_cols
        s = v[:, :D].reshape(M, D // HD, HD)
        es = e[:, :D].reshape(M, D // HD, HD).max(-1, keepdim=True).values
        spread = (s.max(-1, keepdim=True).values - s.min(-1, keepdim=True).values).clamp(max=88.0)
        P = torch.softmax(s, dim=-1)
        eP = P * (2 * es + MARGIN * (2 * U * spread + (HD + 4) * U + (4 * U if c.wlo else UE)))
        v = torch.cat((P.reshape(M, D), v[:, D:]), -1)
        e = torch.cat((eP.reshape(M, D), e[:, D:]), -1)
    if c.act == 1:
        y = _gelu64(v)
        e = 1.13 * e + MARGIN * (0.5 * v.abs() * (4 * U if c.wlo else GELU_AS + UE) + 2 * U * y.abs())
        v = y
    elif c.act == 2:
        v = v.clamp_min(0.0)
    if c.res is not None:
        v = v + c.res[:, :N].double()
        e = e + MARGIN * U * v.abs()
    r = {}
    if c.want_stats:
        t = 64 if c.tile_n == 64 else 128
        pad = (N + t - 1) // t * t - N
        vp, ep = torch.nn.functional.pad(v, (0, pad)), torch.nn.functional.pad(e, (0, pad))
        r["stats"], r["e_stats"] = group_stats(vp, t), group_stats_bound(vp, ep, t)
    sc = c.split_col
    r["out"], r["e"] = (v[:, :sc], e[:, :sc]) if sc else (v, e)
    if c.want_out2:
        r["out2"], r["e2"] = v[:, sc:], e[:, sc:]
    return r


def _trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def gemm_emulate(c, mutant=None):
    """The kernels' rounding contract in plain torch float32: the operand built as the prologue builds it and rounded to bf16
    (or split hi + lo), fp32 accumulation tile by tile over 64-wide K tiles, the epilogue in the order of rg_gemm_epi.h.
    mutant: one of GEMM_MUTANTS, a deliberately wrong variant.  Returns the dict of `gemm_ref` without the bounds
    (bf16 outputs already rounded)."""
    assert mutant is None or mutant in GEMM_MUTANTS
    M, N, K = c.M, c.N, c.K
    f32 = torch.float32
    rnd = _trunc_bf16 if mutant == "trunc_a" else bf16
    rmap = torch.arange(M) % c.a_row_mod if c.a_row_mod else torch.arange(M)
    ng = max(c.groups, 1)
    gw = N // ng
    whi = bf16(c.w)
    wlo = bf16(c.w - whi)
    Kp = (K + 63) // 64 * 64
    Keff = K - (K % 64) if (mutant == "drop_k_tail" and K % 64) else K
    acc = torch.zeros(M, N, dtype=f32)
    for g in range(ng):
        gs = 0 if mutant == "gb_group0" else g
        if c.kind == "bf16":
            a = c.a[:, gs * c.gb_stride:gs * c.gb_stride + K].float()
        elif c.kind == "styl":
            n = torch.tensor(float(K), dtype=f32)
            mu = c.st[..., 0].sum(-1, keepdim=True) / n
            var = (c.st[..., 1].sum(-1, keepdim=True) / n - mu * mu).clamp_min(0.0)
            t = (c.a[:, :K].float() - mu) * torch.rsqrt(var + 1e-5) * c.gain + c.offset
            a = t * torch.sigmoid(t)
        else:
            cols = []
            for i, m in enumerate(c.modes):
                n = min(c.seg_len, K - i * c.seg_len)
                x = c.src[:, c.col[i]:c.col[i] + n].float()
                if m:
                    sl = torch.tensor(float(c.seg_len), dtype=f32)
                    mu = c.stats[i][..., 0].sum(-1, keepdim=True) / sl
                    var = (c.stats[i][..., 1].sum(-1, keepdim=True) / sl - mu * mu).clamp_min(0.0)
                    x = (x - mu) * torch.rsqrt(var + 1e-5) * c.gamma[i][gs][:n] + c.beta[i][gs][:n]
                    if m == 2:
                        x = x * (1.0 if mutant == "styl_noscale" else 1.0 + c.ss[i][:n]) + c.ss[i][c.seg_len:c.seg_len + n]
                        x = x * torch.sigmoid(x)
                cols.append(x)
            a = torch.cat(cols, -1)
        a = a[rmap]
        ah = a if c.kind in ("bf16",) else rnd(a)
        al = bf16(a - ah) if c.wlo else None
        sl_ = slice(g * gw, (g + 1) * gw)
        for k0 in range(0, Keff, 64):
            k1 = min(k0 + 64, Keff)
            if c.wlo:
                acc[:, sl_] += al[:, k0:k1] @ whi[sl_, k0:k1].T
                if mutant != "wlo_no_hilo":
                    acc[:, sl_] += ah[:, k0:k1] @ wlo[sl_, k0:k1].T
            acc[:, sl_] += ah[:, k0:k1] @ whi[sl_, k0:k1].T
    v = acc
    if c.ln:
        kd = torch.tensor(float(Kp if mutant == "ln_kpad" else K), dtype=f32)
        mu = c.ln_stats[..., 0].sum(-1, keepdim=True) / kd
        var = (c.ln_stats[..., 1].sum(-1, keepdim=True) / kd - mu * mu).clamp_min(0.0)
        v = torch.rsqrt(var + 1e-5) * (v - mu * c.c1[None, :])
    if c.bias is not None:
        v = v + c.bias[None, :]
    if c.tb:
        idx = torch.arange(M).clamp_max(c.tb - 1) if mutant == "tbias_row" else torch.arange(M) % c.tb
        v = v + c.tbias[idx]
    if c.softmax_cols:
        D = c.softmax_cols
        o = HD if (mutant == "softmax_shift" and D + HD <= N) else 0        # the mutant: every group one head to the right
        s = v[:, o:o + D].reshape(M, D // HD, HD)
        ex = torch.exp(s - s.max(-1, keepdim=True).values)
        P = (ex * (1.0 / ex.sum(-1, keepdim=True))).reshape(M, D)
        v = torch.cat((v[:, :o], P, v[:, o + D:]), -1)
    if c.act == 1:
        v = 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))
    elif c.act == 2:
        v = v.clamp_min(0.0)
    if c.res is not None:
        if mutant == "res_ldo":                  # rows read at the stride of `out`
            flat = c.res.reshape(-1)
            idx = (torch.arange(M)[:, None] * c.ldo + torch.arange(N)[None, :]) % flat.numel()
            v = v + flat[idx]
        else:
            v = v + c.res[:, :N]
    r = {}
    if c.want_stats:
        t = 64 if c.tile_n == 64 else 128
        pad = (N + t - 1) // t * t - N
        st = group_stats(torch.nn.functional.pad(v, (0, pad)), t)
        r["stats"] = st.roll(1, dims=1) if mutant == "stats_slot" else st
    sc = c.split_col
    out = v[:, :sc] if sc else v
    r["out"] = bf16(out) if c.out_bf16 else out
    if c.want_out2:
        r["out2"] = bf16(v[:, sc:])
    return r


def gemm_cases(num_cus):
    """The cases of test_gemm_kernels_gpu.py (and, at 256 CUs, of test_kernel_refs_cpu.py): name -> constructor.  `variant`
    is the instantiation the dispatch of rg_gemm / rg_gemm_dma_launch reaches for the case (tabulated in the GPU test)."""
    big = lambda N: 64 * -(-(num_cus + 1) // -(-N // 128))          # rows that give more 64 x 128 workgroups than CUs
    C = {}

    def add(name, M, N, K, **kw):
        seed = 7001 + len(C)                     # fixed when the case is added: a later case never reseeds an earlier one
        C[name] = lambda: gemm_case(name, M, N, K, seed, **kw)

    # ---- generic register-staged kernel
    add("g1 ragged K, odd ld, stats ragged N", 65, 160, 78, stats=True, variant="launch<0,0,0>")
    add("g2 one row, ragged tile", 1, 61, 8, path=1, ldo_pad=2, variant="launch<0,0,0>")
    add("g3 LN, tbias 43, residual ldr % 4 != 0, out2", 129, 192, 200, path=1, modes=[1], seg_len=200, nparts=8, tb=43, res=True,
        ldr_pad=3, out2=True, variant="launch<0,0,0>")
    add("g4 4 segments STYL LN IDENT LN short last, gb_group, softmax N", 200, 384, 448, path=1, modes=[2, 1, 0, 1], seg_len=128,
        col0=4, ld_pad=1, groups=3, softmax_cols=384, variant="launch<0,0,0>")
    add("g5 W_lo ragged K, GELU libm", 65, 160, 78, wlo=True, act=1, variant="launch<0,1,0>")
    add("g6 W_lo LN + STYL, softmax 32", 129, 192, 256, path=1, wlo=True, modes=[1, 2], seg_len=128, softmax_cols=32,
        variant="launch<0,1,0>")
    add("g7 bf16 A, folded LN 9 partials, stats", 63, 128, 200, path=1, kind="bf16", ln=9, stats=True, variant="launch<1,0,0>")
    add("g8 bf16 A gb_group, bf16 out at +4 B, ldo % 8 != 0", 200, 256, 256, path=1, kind="bf16", groups=2, out_bf16=True, out_off=2,
        ldo_pad=4, variant="launch<1,0,0>")
    add("g9 split_col 128 ragged rest, odd ldo2", 63, 160, 8, path=1, out2=True, split_col=128, ldo2_pad=3, variant="launch<0,0,0>")
    add("ga full tiles, fp32 ldo % 4 != 0", 65, 128, 8, path=1, ldo_pad=2, variant="launch<0,0,0>")
    add("gb one head N 32, K 512, softmax 32", 64, 32, 512, path=1, softmax_cols=32, variant="launch<0,0,0>")
    add("gc bf16 A K 512, GELU bf16 out streamed", 129, 128, 512, path=1, kind="bf16", act=1, out_bf16=True, variant="launch<1,0,0>")
    add("f1 FAST fp32 A, ReLU bf16 out", 129, 192, 256, path=3, act=2, out_bf16=True, variant="launch<0,0,1>")
    add("f2 FAST bf16 A, a_row_mod, residual, out at +4 B", 65, 256, 512, path=3, kind="bf16", a_row_mod=43, res=True, ldr_pad=4,
        out_off=1, variant="launch<1,0,1>")
    add("f3 FAST fp32 A, tbias 43, softmax N, stats", 65, 128, 256, path=3, tb=43, softmax_cols=128, stats=True, variant="launch<0,0,1>")
    # ---- LDS-DMA kernel, bf16 A
    add("d1 one K tile", 64, 128, 64, kind="bf16", variant="dma_launch<1,0,4,8>")
    add("d2 GELU bf16 out, ragged second tile (path 2)", 65, 160, 128, path=2, kind="bf16", act=1, out_bf16=True,
        variant="dma_launch<1,0,4,8>")
    add("d3 folded LN 4, stats, out2, residual, 3 K tiles (path 5)", 129, 384, 192, path=5, waves=4, kind="bf16", ln=4, stats=True,
        out2=True, res=True, variant="dma_launch<1,0,4,4>")
    add("d4 more workgroups than CUs, 8 waves, ring 2 > K", big(1024), 1024, 64, waves=8, kind="bf16", variant="dma_launch<1,0,2,8>")
    add("d5 more workgroups than CUs, 4 waves, tbias 43, softmax 512 of 1536", big(1536), 1536, 128, waves=4, kind="bf16", tb=43,
        softmax_cols=512, variant="dma_launch<1,0,2,4>")
    add("d6 two workgroups per CU, folded LN 8, residual", big(1024), 1024, 128, kind="bf16", ln=8, res=True, stats=True,
        variant="dma_launch_pair")
    add("d7 two workgroups per CU forced, 5 K tiles", 129, 256, 320, waves=16, kind="bf16", res=True, ldr_pad=8, out2=True,
        variant="dma_launch_pair")
    add("d8 tile_n 64, folded LN 1, stats per 64, out2, residual", 65, 192, 320, kind="bf16", tile_n=64, ln=1, stats=True, out2=True,
        res=True, variant="dma_launch_narrow")
    add("d9 split_col 128 of 256", 129, 256, 512, kind="bf16", out2=True, split_col=128, variant="dma_launch<1,0,4,8>")
    add("da split_col 256 of 320, stats, ReLU", 200, 320, 64, waves=4, kind="bf16", out2=True, split_col=256, stats=True, act=2,
        variant="dma_launch<1,0,4,4>")
    add("db bf16 A gb_group 128, a_row_mod", 129, 256, 128, kind="bf16", groups=2, a_row_mod=43, variant="dma_launch<1,0,4,8>")
    add("dc two workgroups per CU forced, tbias 43, softmax 64", 65, 160, 128, waves=16, kind="bf16", tb=43, softmax_cols=64,
        variant="dma_launch_pair")
    add("dd tile_n 64 one tile N 64, tbias 43, softmax 32", 63, 64, 64, kind="bf16", tile_n=64, tb=43, softmax_cols=32,
        variant="dma_launch_narrow")
    add("de folded LN 9 partials (scalar loop)", 65, 160, 192, kind="bf16", ln=9, stats=True, variant="dma_launch<1,0,4,8>")
    add("df one head N 32", 63, 32, 64, kind="bf16", softmax_cols=32, variant="dma_launch<1,0,4,8>")
    add("dg two workgroups per CU forced, folded LN 9 partials", 129, 128, 128, waves=16, kind="bf16", ln=9,
        variant="dma_launch_pair")
    # ---- LDS-DMA kernel, fp32 A
    add("e1 plain one K tile", 65, 128, 64, variant="dma_launch<0,0,4,8>")
    add("e2 LN 1 partial, softmax 32, tbias 43", 129, 160, 512, modes=[1], seg_len=512, nparts=1, softmax_cols=32, tb=43,
        variant="dma_launch<0,0,4,4>")
    add("e3 4 segments STYL LN IDENT IDENT short last, col_offset", 200, 192, 640, modes=[2, 1, 0, 0], seg_len=192, nparts=8, col0=4,
        ld_pad=4, variant="dma_launch<0,0,3,4>")
    add("e4 4 segments, 8 waves", 65, 128, 704, waves=8, modes=[0, 2, 0, 1], seg_len=192, nparts=1, variant="dma_launch<0,0,3,8>")
    add("e5 LN, more workgroups than CUs, residual, stats", big(1024), 1024, 64, modes=[1], seg_len=64, res=True, stats=True,
        variant="dma_launch<0,0,2,4>")
    add("e6 plain a_row_mod, more workgroups than CUs, 8 waves, out2", big(1024), 1024, 128, waves=8, a_row_mod=big(1024) // 2,
        out2=True, variant="dma_launch<0,0,2,8>")
    add("e7 W_lo LN, 3 K tiles", 129, 160, 192, wlo=True, modes=[1], seg_len=192, variant="dma_launch<0,1,3,4>")
    add("e8 W_lo STYL, softmax 32, GELU libm", 63, 128, 64, wlo=True, modes=[2], seg_len=64, nparts=8, softmax_cols=32, act=1,
        variant="dma_launch<0,1,3,4>")
    add("e9 LN gb_group 128", 65, 384, 256, modes=[1], seg_len=256, groups=3, variant="dma_launch<0,0,4,4>")
    add("ea plain, residual ldr != ldo, out2, stats", 129, 256, 128, res=True, ldr_pad=4, out2=True, stats=True,
        variant="dma_launch<0,0,4,8>")
    add("eb LN, ReLU bf16 out, split_col 128, residual", 65, 256, 192, modes=[1], seg_len=192, act=2, out_bf16=True, out2=True,
        split_col=128, res=True, variant="dma_launch<0,0,4,4>")
    add("ec one narrow tile N 64, GELU bf16 out", 64, 64, 128, act=1, out_bf16=True, variant="dma_launch<0,0,4,8>")
    # ---- LDS-DMA kernel, stylized bf16 A
    add("s1 a_styl 5 K tiles, residual", 129, 160, 320, kind="styl", res=True, ldr_pad=4, variant="dma_launch_styl<5,8>")
    add("s2 a_styl one K tile, 1 partial", 65, 128, 64, kind="styl", nparts=1, variant="dma_launch_styl<5,8>")
    add("s3 a_styl K 512, out2, 8 partials", 63, 128, 512, kind="styl", nparts=8, out2=True, variant="dma_launch_styl<5,8>")
    add("s4 a_styl more workgroups than CUs", big(1024), 1024, 64, kind="styl", nparts=8, variant="dma_launch_styl<3,4>")
    add("s5 a_styl tbias 43, softmax 32, stats", 65, 160, 64, kind="styl", tb=43, softmax_cols=32, stats=True,
        variant="dma_launch_styl<5,8>")
    # ---- 128-row big-tile kernel
    add("b1 128x256 ragged half, folded LN 4, stats, out2, residual", 200, 384, 128, path=4, kind="bf16", ln=4, stats=True, out2=True,
        res=True, variant="big_launch<256>")
    add("b2 128x128 ragged, GELU bf16 out", 129, 192, 320, path=6, kind="bf16", act=1, out_bf16=True, variant="big_launch<128>")
    add("b3 128x128 ring 2, softmax N, tbias 43, split_col 128", 65, 256, 512, path=7, kind="bf16", softmax_cols=256, tb=43, out2=True,
        split_col=128, variant="big_launch<128,2,4>")
    add("b4 128x256 gb_group 256", 129, 512, 192, path=4, kind="bf16", groups=2, variant="big_launch<256>")
    add("b5 128x256 split_col 128 inside the tile, ragged half, a_row_mod", 129, 384, 128, path=4, kind="bf16", out2=True,
        split_col=128, a_row_mod=43,
        variant="big_launch<256>")
    add("b6 128x128 folded LN 9 partials, tbias 43", 200, 256, 128, path=6, kind="bf16", ln=9, tb=43,
        variant="big_launch<128>")
    return C
