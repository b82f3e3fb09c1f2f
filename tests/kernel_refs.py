"""fp64 references, error bounds and fp32 / bf16 emulations for the per-op kernels of csrc/rg_attn.hip and csrc/rg_vae.hip, for
the fused GEMM family (csrc/rg_gemm*.hip, rg_gemm_epi.h), for the stages of the fused stacks (csrc/rg_seq.hip, rg_seq2.hip,
rg_venc.hip, rg_vdec.hip) and for the condition side's fused projection + reduction (csrc/rg_condkv.hip).

Shared by test_attn_kernels_gpu.py, test_vae_kernels_gpu.py, test_gemm_kernels_gpu.py, test_seq_stages_gpu.py, test_venc_stages_gpu.py,
test_vdec_stages_gpu.py, test_cond_kv_gpu.py (kernel vs fp64 reference) and test_kernel_refs_cpu.py (emulation
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

Fused stacks (rg_seq_forward and its launch forms: `seq_*_ref`, `seq_stage_emulate`; rg_venc_forward: `venc_*`; rg_vdec_step: `vdec_*`)
------------------------------------------------------------------------------------------------------------------------------------
The references are teacher-forced: stage s starts from the kernel's own dump of the stage before it, exact fp32 values with
input error 0, so one stage's bound covers one block.  Parameters come from the state dict and the header's formulas (`SeqModel`,
`VencModel`): W diag(gamma) and b + W beta in fp64, the ca_mix fusion, the row sums of its bf16 x block, the stylization gain
gamma (1 + scale) and offset beta (1 + scale) + shift of the sequence's step, the classifier-free rows W_c stylize(value bias).
Unit GEMM (`_lin`): MARGIN (K + n) U sum of magnitudes for the fp32 accumulation onto n initial terms (bias, residual, tables)
+ sum_k E_k |w_k| for an operand within E of the reference's.  Operand tiers at the kernels' bf16 rounding points:
  prologue   (the file's tier) e + half a bf16 ulp at |x| + e: softmaxed q, P and V of the key softmax, A, the stylized y.
  rounded    the panels normalised from a dumped state (xhat) and the classifier-free table rows: their fp32 value is known to a
             few U (`ln_bound`, depth STACK_DEPTH = 26: 16 additions per lane, 2 lane-group steps, 8 waves), so the reference
             rounds them to bf16 ITSELF; the kernel holds the same number unless the value lies within its bound of a rounding
             tie, where it may hold the neighbour, one ulp away (`_rounded`).  This tier is what the prologue tier tightens to
             when the input is exact; without it the score errors put half of the masked stage 11-13 elements within their bound
             of a 1/16-grid tie, and the row-sum identity below drowns.
  exact      raw panels of a dumped state (FFN, head, embedding): bf16 of exact fp32 values, E = 0.
Key softmax (stage 10): scores with errors e_k give P the relative error 2 max e_k + MARGIN e_P (file's e_P, u_exp = 2 UE: the
exp2 and the fast reciprocal); masked and padded tokens weigh exactly 0.  Products of two inexact operands (P^T V, q A) take
sum (E_a |b| + |a| E_b + E_a E_b) + MARGIN n U sum |a| |b|.  Cross attention: A is the bf16 number in the fragments (exact tier);
masked query rows get `ca_ref`'s 1/16-grid treatment.
mix_x (stage 3): the kernel forms x W_x^T + b as sd (bf16(xhat) W_x^T + rstd (mean c1 + b)), c1 = rowsum(bf16(W_x)); the
reference evaluates THAT expression with its own bf16(xhat) (rounded tier), so mean and rstd no longer cancel:
  e = sd e_acc + MARGIN (e_sd |sd acc| + e_mu |c1| + (UE + 2 U) |out|),  e_mu, e_sd = e_var / (2 var) as in "Fused GEMM".
Stylization (`_styl_operand`): `styl_ref` + MARGIN UE |silu| for silu_f's reciprocal.  GELU: the file's GELU_AS + UE term.
Statistical tier (stage 4 of a denoiser layer, every block of rg_venc).  Behind the FFN's hidden layer lie three chained
GEMMs and a LayerNorm between two dumps, behind a VAE block eight roundings.  Worst-case sums over the 1024 half-ulps of the
hidden activations, divided by the row's standard deviation and summed once more over 512 features, put the stage 4 bound at 2
to 8 rms of the signal and a VAE block's at several hundred: a second linear2 bias, a missing bias of one wave or the wrong
step's table pass under them.  These stages are therefore NOT bounded in the worst case.  Their check is a statistical
statement: every rounding is modelled as an independent zero-mean error, variances are propagated to first order and STAT = 2
MARGIN = 8 standard deviations are allowed ONCE, at the end:
  bf16 rounding    var += half_ulp^2 / 3 (uniform within half an ulp; `_r16v`)
  unit GEMM        var_out = var_a (w^2)^T + sum var_init + n (U sum of magnitudes)^2 (`_mmv`: a random walk of n roundings)
  LayerNorm        d y_k = gamma_k / sigma (d x_k - mean(d x) - xhat_k mean(xhat d x)), + e_mu^2, e_var^2 of `ln_bound` (`_lnv`)
  GELU, SiLU       slope^2 var (1.13, 1.1) + the square of the approximation error (GELU_AS + UE; 2 UE + 4 U)
  softmax          d p_j = p_j (d s_j - sum_l p_l d s_l);  products of two inexact operands: var_a b^2 + a^2 var_b
The independence is an assumption and is not verified: roundings of correlated operands are not independent (the error of an
operand that feeds all 1024 hidden units is common to them; a residual and the branch computed from it share their error), and a
systematic error (the GELU fit) enters as if it were random.  What speaks for the model is measured, not proven: a correct
emulation and the kernel sit at 0.3 to 0.45 of the bound at every one of these stages, i.e. their worst element of ~1e5 lies
2.5 to 3.6 model standard deviations out, as a Gaussian maximum would.  The bound is 0.6 to 1.1 % of the rms of the reference.
The CPU mutants (SEQ_MUTANTS, VENC_MUTANTS in test_kernel_refs_cpu.py) are the condition on all of this: each exceeds the bound
at its own stage, on the synthetic model's own parameters.  One of them decides one test input (`off_centre`): rows 1.5 off
centre, so that mean (rowsum(W) - rowsum(bf16(W))) stands out of the accumulation bound of the mix_x unit.
Decoder (rg_vdec_step: one launch per block, a 160-token sequence as four 40-row tiles; launch `step` runs [attention ... norm2 of
block step - 1] -> [skip linear of block step] -> [Q, K, V of block step]).  Between two launches the kernel leaves more than a
dump: the fp32 residual x, the keys and values (bf16, through L2, double-buffered by launch parity) and every tile's Q panel.
Each is teacher-forced on what the launch before it left, so a launch is checked in three tiers:
  skip linear   `vdec_skip_ref`: x behind the skip linear from the two dumped states it concatenates.  WORST CASE (`_lin`): exact
                operands (bf16 of exact fp32), one fp32 accumulation over 2 * 512 products and two bias vectors.
  Q, K, V       `vdec_proj_ref`: Q = K-operand = bf16(fp32(x + pos)), V-operand = bf16(x) with the kernel's own fp32 x and the exact
                pos, the 1 / sqrt(16) folded into W_q and b_q in fp32 as the host does.  WORST CASE: `_lin` with exact operands,
                then `bf16_bounds` for the bf16 stores (the half-ulp form first, then the MARGIN form).
  block, final  `vdec_block_ref`, `vdec_final_ref`: the state behind block b from that x.  STATISTICAL, as `venc_block_ref`, with 32
                heads of 16, S = 160 keys in the softmax term, 2 S roundings in the P V accumulation (P as bf16 hi + lo) and x
                entering the out_proj residual with variance 0 (it is the kernel's own number).
The Q image is the tile's LDS panel as `panel_store` (rg_stationary.h) writes it: bf16 [3 tb][16 s][4 gq][16 l][8 e] = Q[token 40
quarter + 16 tb + l, feature 32 s + 8 gq + e] for tile 4 seq + quarter; rows 16 tb + l >= 40 are padding (`vdec_qimg_rows`).
What the statistical tier does NOT resolve: a defect of a few keys.  `drop_last_keys` (16 of 160) reaches 1.4 to 1.6 of the bound
behind the output blocks on the product's input (12 behind block 0, 10 to 30 on dense rows) -- caught, but a smaller defect in
the attention would not be.  The worst-case checks of K, V and the Q image are what covers that half of a launch: a wrong, stale or
misplaced key, value or query row is 200 to 5e5 bounds out there (`k_no_pos`, `v_with_pos`, `no_scale`), and the parity half a
launch must not write is compared bit for bit.  Both inputs of `vdec_input` keep the correct emulation inside every bound with
the variance model as it stands (0.33 to 0.58 statistical, 0.83 to 0.96 of half a bf16 ulp + accumulation, 1e-4 to 3e-4 skip linear).

Condition side (rg_cond_kv: `cond_kv_case`, `cond_kv_ref`, `cond_kv_emulate`; test_cond_kv_gpu.py)
---------------------------------------------------------------------------------------------------
One launch per condition: [K | V] = xhat W_l^T + b_l for every layer (bf16 operands, fp32 accumulators that start from the bias),
the softmax of K over a clip's N <= 512 tokens, A_h = P^T V per head with the un-normalised P and V as bf16 hi + lo pairs (three
products per 64-token group), the groups' partial matrices added in wave order and scaled by 1 / sum.  The reference takes the
bf16 inputs in fp64.  With S = sum_n P_n |v_n| per (head, key column i, value column j):
    |err A| <= MARGIN (e_P + N U + US) S                          e_P = `_e_p` with u_exp = 2 UE (exp2 and the scaling by 1 / sum)
e_P is the softmax (maximum subtraction, the sum over N, the exponential), N U the fp32 accumulation of the N products and of
the <= 8 partial matrices, US the hi + lo products.  There is NO term for the projection in the `grid` family: its inputs are
multiples of 1/8 (|x| <= 4), 1/64 (|w| <= 1/8) and 1/512 (|b| <= 1/2), so every product and every partial sum of a row's 512 terms
is a multiple of 2^-9 below 2^9 -- 18 bits -- and fp32 accumulation is exact in ANY order (test_kernel_refs_cpu.py compares the
fp32 matmul with the fp64 one bit for bit; that the matrix cores add such terms exactly is supposed -- if the kernel misses this
bound where the emulation meets it, that supposition is the first thing to examine, not the bound).  K and V then enter the
softmax and the reduction with error 0 and the bound resolves the hi + lo products themselves.
The `gauss` family (bf16 randn rows, 0.04 randn weights, one key column per layer scaled to a spread of about +-80: the k-mapping,
the addressing and the maximum subtraction) pays for the projection in the worst case: d = (512 + 1) U (sum_k |x_k| |w_k| + |b|)
per score and per value.  A score error costs P the relative 2 max_n d_K (its own score and the normaliser); V carries d_V:
    |err A| <= MARGIN ((e_P + 2 max_n d_K + N U + US) S + sum_n P_n d_V,n)
This bound is loose by construction (a correct emulation: 3e-4 to 2e-3 of it) and is there for the gross errors.
The `zeros` family (xhat = 0: the one-speaker model's condition rows) has K = b_K for every token, so P = 1 / N and
A[l, b, h, i, j] = b_V[l, 32 h + j] for every i, within the grid bound.
Measured on the CPU, worst |err| / bound over the 17 shapes of COND_KV_CASES (N = 1 .. 512, every wave split 1 .. 8):
  correct emulation   grid 0.0018 (N = 1), 0.19 (N = 2), 0.12 .. 0.09 (N = 63 .. 150), 0.06 .. 0.025 (N = 192 .. 512);  gauss 3e-4 .. 2e-3
  hi_only             grid 59 (N = 1), 80 (N = 2), 54 .. 33 (N = 64 .. 150), 28 .. 12 (N = 192 .. 512);  gauss 0.14 .. 1.0: NOT resolved there
  pad_rows_counted    grid 3.2e5 (N = 2), 5.4e3 (N = 63), 1.5e5 (N = 65), 7e3 .. 7e4 beyond;  gauss 114 .. 595
  max_per_group       grid 3e4 .. 2e6;  gauss 101 .. 402          sum_of_slot0    grid 2.4e4 .. 4.7e4;  gauss 334 .. 414
  bias_of_layer0      grid 6e4 .. 1.3e5;  gauss 102 .. 120        heads_swapped, a_transposed    grid > 1e5;  gauss 475 .. 2e3
The kernel on the MI355X sits where the emulation does (grid 0.0031 at N = 1, 0.19 at N = 2, 0.12 .. 0.025 from N = 63 to 512; gauss
2.8e-4 .. 1.9e-3; zeros 2e-11): the grid family needed no accumulation term, so the matrix cores did add its terms exactly.
A mutant applies where it computes something else (`cond_kv_mutant_applies`): pad_rows_counted needs N % 64 != 0, max_per_group
N > 64, sum_of_slot0 two clips in a workgroup, bias_of_layer0 L >= 2 -- and the first and third need N >= 2: with one token the
softmax is 1 whatever else is counted, the copies of the row in the pad rows weigh 64 x 1/64 and every clip's column sum is 1.0.
"""
import types

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


# ----------------------------------------------------------------------------------------------- condition side (rg_cond_kv)
# (derivation of the bound: module docstring, "Condition side")
COND_DM, COND_H, COND_WAVES = 512, 16, 8
COND_KV_FAMILIES = ("grid", "gauss", "zeros")
COND_KV_MUTANTS = ("pad_rows_counted", "hi_only", "max_per_group", "sum_of_slot0", "heads_swapped", "bias_of_layer0", "a_transposed")
LOG2E = 1.44269504088896340736
# (N tokens, B clips, L layers), by wave split and clip packing: wpc 1 (cpw 8) | wpc 2 | wpc 3, two idle waves | wpc 4 | wpc 5 to 7,
# idle waves, one clip per workgroup | wpc 8.  B is chosen so that the last workgroup is partly filled in most of them.
COND_KV_CASES = ((1, 9, 1), (2, 1, 1), (63, 3, 1), (64, 8, 1), (65, 5, 1), (128, 4, 1), (129, 3, 1), (150, 3, 3), (192, 2, 1), (193, 3, 1),
                 (257, 2, 1), (321, 1, 1), (385, 1, 1), (448, 1, 1), (449, 2, 1), (499, 2, 2), (512, 1, 1))
COND_KV_GAUSS_CASES = ((1, 9, 1), (65, 5, 1), (150, 3, 3), (257, 2, 1), (499, 2, 2))
COND_KV_ZEROS_CASES = ((65, 5, 1),)
COND_KV_RUNS = tuple([c + ("grid",) for c in COND_KV_CASES] + [c + ("gauss",) for c in COND_KV_GAUSS_CASES]
                     + [c + ("zeros",) for c in COND_KV_ZEROS_CASES])


def cond_kv_seed(N, B, L, family):
    return 7000 + 10 * N + B + 3 * L + 5000 * COND_KV_FAMILIES.index(family)


def cond_kv_split(N):
    """(wpc, cpw): waves per clip and clips per workgroup of rg_cond_kv at N tokens per clip."""
    wpc = (N + 63) // 64
    return wpc, COND_WAVES // wpc


def cond_kv_mutant_applies(mutant, N, B, L):
    """Whether the wrong variant computes something else than the kernel at this shape.  A clip of ONE token is degenerate:
    softmax over one token is 1 whatever is counted beside it, so its copies in the pad rows (each weighing 1 / 64 of the same
    value row) and the neighbouring clip's column sums (1.0 like its own) change nothing."""
    wpc, cpw = cond_kv_split(N)
    return {"pad_rows_counted": N % 64 != 0 and N >= 2, "max_per_group": N > 64, "sum_of_slot0": cpw >= 2 and B >= 2 and N >= 2,
            "bias_of_layer0": L >= 2}.get(mutant, True)


def _grid_ints(g, shape, lo, hi, step):
    return torch.from_numpy(g.integers(lo, hi + 1, shape).astype(np.float32)) * step


def cond_kv_case(N, B, L, family, seed):
    """Inputs of one rg_cond_kv problem on the CPU: xhat bf16 [B, N, 512], w bf16 [L, 1024 (key | value), 512], bias fp32 [L, 1024]
    (fields of the returned namespace, with N, B, L, family).
    grid   xhat = multiples of 1/8 in [-4, 4], w = multiples of 1/64 in [-1/8, 1/8], bias = multiples of 1/512 in [-1/2, 1/2]: every
           product and every partial sum of the projection is a multiple of 2^-9 below 2^9 (512 * 4 / 8 + 1/2), i.e. exact in fp32
           in any order.
    gauss  xhat = bf16(randn), w = bf16(0.04 randn), bias = 0.1 randn; the weight row of key column 5 of every layer is scaled by 30, so
           that this column's keys spread over about +-80.
    zeros  xhat = 0 (the one-speaker model's condition rows), w and bias of the grid family."""
    assert family in COND_KV_FAMILIES and 1 <= N and 1 <= B and 1 <= L
    g = rng(seed)
    c = types.SimpleNamespace(N=N, B=B, L=L, family=family, _acc={})
    if family == "gauss":
        x = torch.from_numpy(g.standard_normal((B, N, COND_DM)).astype(np.float32))
        w = torch.from_numpy((0.04 * g.standard_normal((L, 2 * COND_DM, COND_DM))).astype(np.float32))
        w[:, 5] *= 30.0
        c.bias = torch.from_numpy((0.1 * g.standard_normal((L, 2 * COND_DM))).astype(np.float32))
    else:
        x = _grid_ints(g, (B, N, COND_DM), -32, 32, 1.0 / 8)
        w = _grid_ints(g, (L, 2 * COND_DM, COND_DM), -8, 8, 1.0 / 64)
        c.bias = _grid_ints(g, (L, 2 * COND_DM), -256, 256, 1.0 / 512)
        if family == "zeros":
            x = torch.zeros_like(x)
    c.xhat, c.w = x.to(torch.bfloat16), w.to(torch.bfloat16)
    if family != "gauss":
        assert torch.equal(c.xhat.float(), x) and torch.equal(c.w.float(), w)
    return c


def _cond_heads(kv, L, B, N):
    """[L, B, N, 1024] -> keys, values [L, B, N, 16, 32]."""
    return kv[..., :COND_DM].reshape(L, B, N, COND_H, HD), kv[..., COND_DM:].reshape(L, B, N, COND_H, HD)


def cond_kv_ref(c):
    """A[l][b][h] = softmax_N(K_h)^T V_h, [K | V] = xhat W_l^T + b_l, in fp64 from the bf16 numbers.  Returns (A [L, B, 16, 32, 32],
    bound): MARGIN (sum_n P (e_P + N U + US) |v|), e_P with u_exp = 2 UE; the gauss family adds the projection's accumulation
    d = (512 + 1) U (sum |x| |w| + |b|): 2 max_n d_K relative on P and sum_n P d_V (module docstring, "Condition side")."""
    L, B, N = c.L, c.B, c.N
    x, w = c.xhat.double().view(B * N, COND_DM), c.w.double().view(L * 2 * COND_DM, COND_DM)
    kv = (x @ w.T).view(B, N, L, 2 * COND_DM).permute(2, 0, 1, 3) + c.bias.double()[:, None, None, :]
    k, v = _cond_heads(kv, L, B, N)
    P = torch.softmax(k, dim=2)
    pv = lambda p, u: torch.einsum("zbnhd,zbnhj->zbhdj", p, u)
    A = pv(P, v)
    rel = _e_p(k.reshape(L * B, N, COND_H, HD), torch.ones(L * B, N, dtype=torch.bool), N, 2 * UE).view(L, B, COND_H, HD) + N * U + US
    extra = 0.0
    if c.family == "gauss":
        d = (COND_DM + 1) * U * ((x.abs() @ w.abs().T).view(B, N, L, 2 * COND_DM).permute(2, 0, 1, 3) + c.bias.double().abs()[:, None, None, :])
        dk, dv = _cond_heads(d, L, B, N)
        rel = rel + 2 * dk.max(dim=2).values
        extra = pv(P, dv)
    return A, MARGIN * (rel[..., None] * pv(P, v.abs()) + extra)


def _cond_project_f32(c, layer0_bias):
    """fp32 [K | V] [L, B, N, 1024] as the kernel accumulates them: from the bias, sixteen 32-deep steps, step 2 t over
    k = 64 t + 16 g + [0, 8), step 2 t + 1 over k = 64 t + 16 g + [8, 16) (g = 0..3)."""
    if layer0_bias not in c._acc:
        bias = c.bias[:1].expand(c.L, -1) if layer0_bias else c.bias
        x, w = c.xhat.float(), c.w.float()
        acc = bias[:, None, None, :].expand(c.L, c.B, c.N, 2 * COND_DM).clone()
        for s in range(16):
            ks = (64 * (s >> 1) + 16 * torch.arange(4)[:, None] + 8 * (s & 1) + torch.arange(8)[None, :]).reshape(-1)
            acc += torch.einsum("bnk,zck->zbnc", x[..., ks], w[..., ks])
        c._acc[layer0_bias] = acc
    return c._acc[layer0_bias]


def cond_kv_emulate(c, mutant=None):
    """rg_cond_kv's rounding contract in plain torch float32, in the kernel's order: accumulators from the bias; the clip's column
    maximum over its valid tokens; exp2(fma(k, log2e, -max log2e)) (the fused multiply-add through fp64: the product is exact
    there); column sums per lane (16 rows), lane groups pairwise, 64-token groups in wave order; un-normalised P and V as bf16
    hi + lo, lo hi + hi lo + hi hi per 32-token step chained over the two steps of a 64-token group; the groups' partial
    matrices added in wave order, then rows times 1 / sum.  Rows past N hold row N - 1 and weigh 0.
    mutant: one of COND_KV_MUTANTS, a deliberately wrong variant.  Returns fp32 A [L, B, 16, 32, 32]."""
    assert mutant is None or mutant in COND_KV_MUTANTS
    L, B, N = c.L, c.B, c.N
    wpc, cpw = cond_kv_split(N)
    f32 = torch.float32
    kv = _cond_project_f32(c, mutant == "bias_of_layer0")
    rows = torch.arange(wpc * 64)
    kv = kv[:, :, rows.clamp_max(N - 1)]
    k, v = _cond_heads(kv, L, B, wpc * 64)
    k, v = k.reshape(L, B, wpc, 64, COND_H, HD), v.reshape(L, B, wpc, 64, COND_H, HD)
    valid = (rows < N) | (mutant == "pad_rows_counted")
    valid = valid.view(1, 1, wpc, 64, 1, 1)
    m = torch.where(valid, k, torch.full_like(k, -float("inf"))).amax(dim=3, keepdim=True)          # per 64-token group
    if mutant != "max_per_group":
        m = m.amax(dim=2, keepdim=True)
    l2e = torch.tensor(LOG2E, dtype=f32)
    nm2 = m * -l2e
    e = torch.exp2((k.double() * l2e.double() + nm2.double()).float())
    e = torch.where(valid, e, torch.zeros_like(e))
    el = e.view(L, B, wpc, 4, 4, 4, COND_H, HD)             # row 16 rb + 4 g4 + r of the group
    s = torch.zeros(L, B, wpc, 4, COND_H, HD, dtype=f32)
    for rb in range(4):
        for r in range(4):
            s = s + el[:, :, :, rb, :, r]
    s = (s[:, :, :, 0] + s[:, :, :, 1]) + (s[:, :, :, 2] + s[:, :, :, 3])
    tot = torch.zeros(L, B, COND_H, HD, dtype=f32)
    for wv in range(wpc):
        tot = tot + s[:, :, wv]
    cinv = 1.0 / tot
    if mutant == "sum_of_slot0":
        cinv = cinv[:, torch.arange(B) // cpw * cpw]
    ph, pl = split_hi_lo(e)
    vh, vl = split_hi_lo(v)
    A = torch.zeros(L, B, COND_H, HD, HD, dtype=f32)
    pv = lambda p, u, wv, t: torch.einsum("zbnhd,zbnhj->zbhdj", p[:, :, wv, t:t + 32], u[:, :, wv, t:t + 32])
    for wv in range(wpc):
        part = torch.zeros_like(A)
        for t in (0, 32):
            if mutant != "hi_only":
                part = part + pv(pl, vh, wv, t)
                part = part + pv(ph, vl, wv, t)
            part = part + pv(ph, vh, wv, t)
        A = part if wv == 0 else A + part
    A = A * cinv[..., None]
    if mutant == "heads_swapped":
        A = A.view(L, B, COND_H // 2, 2, HD, HD).flip(3).reshape(L, B, COND_H, HD, HD)
    if mutant == "a_transposed":
        A = A.transpose(-1, -2)
    return A.contiguous()


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


# ----------------------------------------------------------------------------------------------- fused stacks (rg_seq, rg_venc)
# (derivation of the bounds: module docstring, "Fused stacks")
DM = 512
STACK_DEPTH = 26          # one-pass row statistics: up to 16 additions per lane, 2 lane-group steps, 8 waves
LOG2E = 1.4426950408889634
SEQ_CONDS = ("xf_text", "xf_audio", "xf_spk")
SEQ_STAGES = (10, 2, 11, 12, 13, 3, 4)          # the order in which a layer passes them
# deliberately wrong variants of the emulations -> the stage that has to catch them
SEQ_MUTANTS = dict(bias_wave1=2, pad_rows=10, masked_token=10, styl_step=2, no_grid=12, a_blocks_swapped=11, ff2_bias_twice=4,
                   rowsum_fp32=3, unc_flag=3, ffo_bias_wave1=4, ffo_bias_none=4, ff1_bias_wave1=4, ffn_styl_step=4)
VENC_MUTANTS = ("no_scale", "skip_swapped", "norm2_for_norm1")


STAT = 2 * MARGIN          # standard deviations of the variance model that a bound of the statistical tier allows


def _wb(w):
    """What the matrix cores multiply: the fp32 weight rounded to bf16, as fp64."""
    return bf16(w.float()).double()


def _lin(a, Ea, w, inits=()):
    """sum(inits) + a w^T with fp32 accumulation over K + len(inits) terms; Ea: distance bound of the operand (or None)."""
    out, mag = a @ w.T, a.abs() @ w.abs().T
    for i in inits:
        out, mag = out + i, mag + i.abs()
    e = MARGIN * (a.shape[-1] + len(inits)) * U * mag
    return out, (e + Ea @ w.abs().T if Ea is not None else e)


def _r16v(x, var):
    """Variance after a rounding to bf16: uniform within half an ulp."""
    h = bf16_half_ulp(x.abs() + STAT * torch.sqrt(var))
    return var + h * h / 3


def _mmv(a, va, w, inits=()):
    """sum(inits) + a w^T with the variances of independent operand errors va (None: exact) and inits [(value, variance or
    None)]; the fp32 accumulation walks n = K + len(inits) roundings of at most U times the sum of magnitudes each."""
    out, mag = a @ w.T, a.abs() @ w.abs().T
    var = va @ (w * w).T if va is not None else torch.zeros_like(out)
    for iv, ivar in inits:
        out, mag = out + iv, mag + iv.abs()
        if ivar is not None:
            var = var + ivar
    return out, var + (a.shape[-1] + len(inits)) * (U * mag) ** 2


def _lnv(x, var, gb):
    """LayerNorm with affine from one-pass statistics (row_stats_vae), first order: d y_k = gamma_k / sigma (d x_k - mean(d x) -
    xhat_k mean(xhat d x)) for independent d x, + the statistics' own rounding (e_mu, e_var of `ln_bound`) + the output's."""
    n = x.shape[-1]
    mu, msq = x.mean(-1, keepdim=True), (x * x).mean(-1, keepdim=True)
    sig = torch.sqrt((msq - mu * mu).clamp_min(0.0) + 1e-5)
    xh = (x - mu) / sig
    y = xh * gb[0] + gb[1]
    e_mu = STACK_DEPTH * U * x.abs().mean(-1, keepdim=True)
    e_var = STACK_DEPTH * U * msq + 2 * mu.abs() * e_mu
    vin = var + var.mean(-1, keepdim=True) / n + xh * xh * (xh * xh * var).mean(-1, keepdim=True) / n + e_mu ** 2 + (xh * e_var / (2 * sig)) ** 2
    return y, (gb[0] / sig) ** 2 * vin + (4 * U) ** 2 * ((xh * gb[0]) ** 2 + y * y + gb[1] ** 2)


def _prologue(x, e):
    """The "prologue" tier: the kernel rounds an fp32 value within e of x to bf16."""
    return x, e + bf16_half_ulp(x.abs() + e)


def _rounded(x, e):
    """The reference rounds x to bf16 itself: the kernel, whose fp32 value lies within e of x, holds the same bf16 number unless
    x is within e of a rounding tie -- there it may hold the neighbour, one ulp away.  Returns (bf16(x), distance bound)."""
    xb = bf16(x.float()).double()
    ax, axb = x.abs(), xb.abs()
    h_up = bf16_half_ulp(axb)
    pow2 = axb == torch.exp2(torch.floor(torch.log2(axb.clamp_min(2.0 ** -126))))
    h_lo = torch.where(pow2, h_up / 2, h_up)
    d = ax - axb
    tie = torch.minimum(h_up - d, d + h_lo) <= e
    return xb, torch.where(tie, 2 * bf16_half_ulp(ax + e), torch.zeros_like(x))


def _xhat_ref(X):
    """(x - mean) rstd of the fp32 rows X from one-pass statistics (no affine: it is folded into the weights); bound with margin."""
    one, zero = torch.ones(X.shape[-1], dtype=F64), torch.zeros(X.shape[-1], dtype=F64)
    return styl_ref(X, 0.0, one, zero, None, None, STACK_DEPTH)


def _styl_operand(y, e, gamma, beta, scale, shift, tier=None):
    """The stylized bf16 panel SiLU(LN(y) (1 + scale) + shift) (silu_f: exp2 and a fast reciprocal, UE each); e without the margin."""
    s, es = styl_ref(y, e, gamma, beta, scale, shift, STACK_DEPTH)
    return (tier or _prologue)(s, es + MARGIN * UE * s.abs())


def _softmax32_ref(q, eq):
    """rg_softmax32 over each head's 32 features of q [..., 512] with element bounds eq; returns the bf16 operand tier."""
    sh = q.shape
    s, es = q.reshape(*sh[:-1], sh[-1] // HD, HD), eq.reshape(*sh[:-1], sh[-1] // HD, HD).max(-1, keepdim=True).values
    spread = (s.max(-1, keepdim=True).values - s.min(-1, keepdim=True).values).clamp(max=88.0)
    P = torch.softmax(s, dim=-1)
    eP = P * (2 * es + MARGIN * (2 * U * spread + (HD + 4) * U + 2 * UE))
    return _prologue(P.reshape(sh), eP.reshape(sh))


def _ffn_hidden_var(a, va, w1, b1, w2, inits):
    """inits + gelu_fast(a w1^T + b1) w2^T with variances: one half of a hidden layer (statistical tier).  The hidden activations
    are rounded to bf16; the GELU's approximation error enters as if it were one more standard deviation."""
    h, vh = _mmv(a, va, w1, [(b1, None)])
    g = _gelu64(h)
    vg = _r16v(g, 1.13 ** 2 * vh + (0.5 * h.abs() * (GELU_AS + UE) + 2 * U * g.abs()) ** 2)
    return _mmv(g, vg, w2, inits)


class SeqModel:
    """fp64 parameters of the denoiser's decoder layers, straight from the reference state dict (g(name) -> fp32 CPU tensor),
    the AdaLN table ss [S, L, 5, 2 D] (scale | shift per step, layer and stylization block) and the header's formulas: folded
    LayerNorm gains, the ca_mix fusion, its row sums.  Nothing here reads a packed stream."""

    def __init__(self, g, ss, L, T):
        D = DM
        d = lambda n: g(n).double()
        self.L, self.T, self.ss = L, T, ss.double().cpu()
        n_lat = (T - 3) // 4
        pos, sep = d("sequence_embedding.pe").permute(1, 0, 2)[0, :n_lat], torch.zeros(1, D, dtype=F64)
        self.tbias = (torch.cat([pos, sep, pos, sep, pos, sep, pos]) + d("global_positional_embedding.pe")[:T, 0]).float().double()
        self.embed = (_wb(d("joint_embed.weight")), d("joint_embed.bias"))
        self.head = (_wb(d("out.weight")), d("out.bias"))

        def fold(p):       # LN(x) W^T + b = xhat (W diag(gamma))^T + (b + W beta)
            w, b, ga, be = d(p + "weight"), d(p + "bias"), d(p.rsplit(".", 2)[0] + ".norm.weight"), d(p.rsplit(".", 2)[0] + ".norm.bias")
            return _wb(w * ga[None, :]), (b + w @ be).float().double()

        self.layers = []
        for l in range(L):
            p = "temporal_decoder_blocks.%d." % l
            sa = p + "sa_block."
            lw = dict(q=fold(sa + "query."), k=fold(sa + "key."), v=fold(sa + "value."),
                      sao=(_wb(d(sa + "proj_out.out_layers.2.weight")), d(sa + "proj_out.out_layers.2.bias")),
                      styl=[(d(sa + "proj_out.norm.weight"), d(sa + "proj_out.norm.bias"))])
            wm, bias = d(p + "ca_mix.weight"), d(p + "ca_mix.bias")
            lw["q3"], lw["mix"], lw["bv"] = [], [], []
            for c, cn in enumerate(SEQ_CONDS):
                ca = p + "ca_blocks.%s." % cn
                wmc = wm[:, c * D:(c + 1) * D]
                lw["q3"].append(fold(ca + "query."))
                lw["mix"].append(_wb(wmc @ d(ca + "proj_out.out_layers.2.weight")))
                bias = bias + wmc @ d(ca + "proj_out.out_layers.2.bias")
                lw["styl"].append((d(ca + "proj_out.norm.weight"), d(ca + "proj_out.norm.bias")))
                lw["bv"].append(d(ca + "value.bias"))
            wx = (wm[:, :D] + wm[:, D:2 * D] + wm[:, 2 * D:]).float().double()
            lw["wx"], lw["wx32"], lw["b_mix"] = _wb(wx), wx, bias.float().double()
            lw["c1"] = lw["wx"].sum(1).float().double()                 # row sums of the bf16 weight
            w1, w2 = d(p + "ffn.linear1.weight"), d(p + "ffn.linear2.weight")
            lw["ff1"] = [(_wb(w1[j * D:(j + 1) * D]), d(p + "ffn.linear1.bias")[j * D:(j + 1) * D]) for j in range(2)]
            lw["ff2"] = [_wb(w2[:, j * D:(j + 1) * D]) for j in range(2)]
            lw["b_ff2"] = d(p + "ffn.linear2.bias")
            lw["ffo"] = (_wb(d(p + "ffn.proj_out.out_layers.2.weight")), d(p + "ffn.proj_out.out_layers.2.bias"))
            lw["styl"].append((d(p + "ffn.proj_out.norm.weight"), d(p + "ffn.proj_out.norm.bias")))
            self.layers.append(lw)

    def ss_rows(self, st, l, bi):
        """(scale, shift) [R, 1, D] of stylization block bi (0 self attention, 1-3 cross attention, 4 FFN) at the steps st [R]."""
        t = self.ss[st, l, bi]
        return t[:, None, :DM], t[:, None, DM:]


def seq_case(B, T, seed, step=49, step_b=None, split=None, L=2):
    """Inputs of one launch, on the CPU: B, T, L; x [B, T, 512]; mm [B, T], qm [3, B, T] and their doubled forms src_mask
    [2 B, T], qmask [3, 2 B, T]; A [L, 3, B, 16, 32, 32]; step, step_b, split; st [2 B] = the step index of every sequence.
    Masks as tests/test_seq_twin_gpu.py: masked motion tokens, masked query rows of every condition in the first and in the
    last token block, and (B > 1) one clip with every token masked."""
    c = types.SimpleNamespace()
    c.B, c.T, c.L, c.step = B, T, L, step
    c.step_b, c.split = (step if step_b is None else step_b), (B if split is None else split)
    c.x = randn((B, T, DM), seed)
    c.A = randn((L, 3, B, 16, HD, HD), seed + 1, 0.15)
    n = (T - 3) // 4
    mm = torch.ones(B, T)
    mm[:, [n, 2 * n + 1, 3 * n + 2]] = 0
    mm[B - 1, T - 5:] = 0
    if B > 1:
        mm[B - 2, T - 5:] = 0
        mm[B - 1] = 0
    qm = torch.ones(3, B, T)
    for k in range(3):
        qm[k][:, [n, 2 * n, 3 * n]] = 0
        qm[k][0, k] = 0
        qm[k][B - 1, T - 1 - k] = 0
    c.mm, c.qm = mm, qm
    c.src_mask, c.qmask = torch.cat([mm, mm]), torch.cat([qm, qm], dim=1)
    clip = torch.arange(2 * B) % B
    c.st = torch.where(clip >= c.split, torch.tensor(c.step_b), torch.tensor(c.step))
    return c


def off_centre(state, shift=1.5):
    """A copy of a denoiser state dict whose embedding puts every row of the residual stream `shift` off centre (one to two of
    its standard deviations): what the one-pass variance and the row-sum identity of the mix_x unit are sensitive to.  Nothing
    else of the synthetic model is touched."""
    sd = dict(state)
    sd["joint_embed.bias"] = state["joint_embed.bias"] + shift
    return sd


# ---- references of the stages: every one takes the kernel's own dump of the stage before it (exact fp32 values)
def seq_embed_ref(m, c):
    """Stage 1: joint_embed(x) + positional tables, the same rows for a clip's two sequences."""
    w, b = m.embed
    out, e = _lin(bf16(c.x).double(), None, w, [m.tbias[None], b])
    return torch.cat([out, out]), torch.cat([e, e])


def seq_sa_y_ref(m, c, l, X):
    """Stage 10: y = softmax(q) (softmax_N(K)^T V) of the self attention from the state X [R, T, 512]."""
    lw = m.layers[l]
    R, T = X.shape[:2]
    H = DM // HD
    a, Ea = _rounded(*_xhat_ref(X))
    (k, ek), (v, ev), (q, eq) = (_lin(a, Ea, *lw[n][:1], [lw[n][1]]) for n in ("k", "v", "q"))
    valid = c.src_mask != 0
    k4, v4 = k.view(R, T, H, HD), v.view(R, T, H, HD)
    vm = valid[:, :, None, None]
    kk = torch.where(vm, k4, torch.full_like(k4, -float("inf")))
    mx = kk.max(dim=1, keepdim=True).values
    ex = torch.where(vm, torch.exp(kk - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))), torch.zeros_like(k4))
    s = ex.sum(dim=1, keepdim=True)
    P = ex / torch.where(s > 0, s, torch.ones_like(s))
    dk = torch.where(vm, ek.view(R, T, H, HD), torch.zeros_like(k4)).max(dim=1).values
    e_rel = 2 * dk + MARGIN * _e_p(k4, valid, T, 2 * UE)                       # [R, H, 32]
    _, EP = _prologue(P, P * e_rel[:, None])
    EP = torch.where(vm, EP, torch.zeros_like(EP))                              # masked and padded tokens weigh exactly 0
    _, EV = _prologue(v4, ev.view(R, T, H, HD))
    pv = lambda p_, v_: torch.einsum("rthd,rthl->rhdl", p_, v_)
    A = pv(P, v4)
    eA = pv(EP, v4.abs()) + pv(P, EV) + pv(EP, EV) + MARGIN * 48 * U * pv(P, v4.abs())
    _, EA = _prologue(A, eA)
    Q, EQ = _softmax32_ref(q, eq)
    Q, EQ = Q.view(R, T, H, HD), EQ.view(R, T, H, HD)
    qa = lambda q_, a_: torch.einsum("rthd,rhdl->rthl", q_, a_)
    y = qa(Q, A)
    ey = qa(EQ, A.abs()) + qa(Q, EA) + qa(EQ, EA) + MARGIN * HD * U * qa(Q, A.abs())
    return y.reshape(R, T, DM), ey.reshape(R, T, DM)


def _styl_unit_ref(m, c, l, bi, X, eX, y, ey, wb):
    """X + b + stylize(y) W^T (stylization block bi): the units behind the attentions."""
    ga, be = m.layers[l]["styl"][bi]
    sc, sh = m.ss_rows(c.st[:y.shape[0]], l, bi)
    s, Es = _styl_operand(y, ey, ga, be, sc, sh)
    out, e = _lin(s, Es, wb[0], [X, wb[1]])
    return out, e + eX


def seq_sa_out_ref(m, c, l, X, y):
    """Stage 2: X + proj_out(stylize(y)) from the state X and the dumped y of stage 10."""
    return _styl_unit_ref(m, c, l, 0, X, 0.0, y, 0.0, m.layers[l]["sao"])


def seq_ca_y_ref(m, c, l, cond, X2):
    """Stage 11 + cond: y = softmax(q_c) A_c of the conditional sequences X2 [B, T, 512]; masked query rows on the 1/16 grid.
    Returns (y, bound, tie: masked elements that may land one grid step away)."""
    lw = m.layers[l]
    B, T = X2.shape[:2]
    H = DM // HD
    a, Ea = _rounded(*_xhat_ref(X2))
    q, eq = _lin(a, Ea, lw["q3"][cond][0], [lw["q3"][cond][1]])
    Q, EQ = _softmax32_ref(q, eq)
    Q, EQ = Q.view(B, T, H, HD), EQ.view(B, T, H, HD)
    A = bf16(c.A[l, cond]).double()                                             # the fragments hold bf16(A)
    qa = lambda q_, a_: torch.einsum("rthd,rhdl->rthl", q_, a_)
    y = qa(Q, A).reshape(B, T, DM)
    e = (qa(EQ, A.abs()) + MARGIN * HD * U * qa(Q, A.abs())).reshape(B, T, DM)
    msk = (c.qm[cond] == 0)[:, :, None].expand_as(y)
    tie = msk & near_tie(y, e)
    e = torch.where(msk, torch.where(tie, torch.full_like(e, 1.0 / 16), torch.zeros_like(e)), e)
    return torch.where(msk, grid16(y), y), e, tie


def _mix_x_ref(lw, X2):
    """x W_x^T + b as the kernel forms it: sd (bf16(xhat) W_x^T + rstd (mean rowsum(W_x) + b)).  The reference rounds xhat to bf16
    itself (`_rounded`): the identity's row-sum term is two orders below a half-ulp bound."""
    xh, exh = _xhat_ref(X2)
    mu, msq = X2.mean(-1, keepdim=True), (X2 * X2).mean(-1, keepdim=True)
    var = (msq - mu * mu).clamp_min(0.0)
    sd = torch.sqrt(var + 1e-5)
    e_mu = STACK_DEPTH * U * X2.abs().mean(-1, keepdim=True)
    e_sd = (STACK_DEPTH * U * msq + 2 * mu.abs() * e_mu) / (2 * (var + 1e-5))     # relative
    a, Ea = _rounded(xh, exh)
    c1, b = lw["c1"][None, None], lw["b_mix"][None, None]
    acc, e_acc = _lin(a, Ea, lw["wx"], [mu * c1 / sd, b / sd])
    out = sd * acc
    return out, sd * e_acc + MARGIN * (e_sd * (sd * (a @ lw["wx"].T)).abs() + e_mu * c1.abs() + (UE + 2 * U) * out.abs())


def unc_rows_ref(m, l, cond, st):
    """The classifier-free sequences' cross-attention term of condition `cond` at the steps st [n]: W_c stylize(y) with y the
    value bias (every token attends to the null condition), or its 1/16-grid rounding where the query is masked.
    Returns (rows [n, 2 (unmasked | masked), 512], bound)."""
    lw = m.layers[l]
    bv = lw["bv"][cond].float()
    y = torch.stack([bv, (bv + torch.tensor(-1000000.0)) + torch.tensor(1000000.0)]).double()      # exact fp32 arithmetic
    ga, be = lw["styl"][1 + cond]
    t = m.ss[st, l, 1 + cond]
    s, Es = _styl_operand(y[None], 0.0, ga, be, t[:, None, :DM], t[:, None, DM:], _rounded)
    out, e = _lin(s, Es, lw["mix"][cond])
    return out, e + U * out.abs()


def seq_mix_ref(m, c, l, X2, y3):
    """Stage 3: ca_mix over [h_text | h_audio | h_spk | x] from the state X2 [R, T, 512] and the dumped y of stages 11-13
    (y3: three [B, T, 512]); the classifier-free sequences take their constant rows."""
    lw = m.layers[l]
    B, T = c.B, X2.shape[1]
    out, e = _mix_x_ref(lw, X2)
    mag = out.abs()
    terms = []
    for cond in range(3):
        ga, be = lw["styl"][1 + cond]
        sc, sh = m.ss_rows(c.st[:B], l, 1 + cond)
        s, Es = _styl_operand(y3[cond], 0.0, ga, be, sc, sh)
        tc, ec = _lin(s, Es, lw["mix"][cond])
        rows, er = unc_rows_ref(m, l, cond, c.st[B:])                            # [B, 2, 512]
        flag = (c.qm[cond] == 0).long()                                           # [B, T]
        idx = flag[:, :, None].expand(B, T, DM)
        tu, eu = torch.gather(rows, 1, idx), torch.gather(er, 1, idx)
        terms.append((torch.cat([tc, tu]), torch.cat([ec, eu])))
    for tc, ec in terms:
        out, e, mag = out + tc, e + ec, mag + tc.abs()
    return out, e + MARGIN * 4 * U * mag


def seq_ffn_ref(m, c, l, X3):
    """Stage 4: X3 + proj_out(stylize(linear2(gelu(linear1(X3))))), the 1024 hidden units in two halves."""
    lw = m.layers[l]
    a = bf16(X3).double()
    y, vy = _ffn_hidden_var(a, None, *lw["ff1"][0], lw["ff2"][0], [(lw["b_ff2"], None)])
    y, vy = _ffn_hidden_var(a, None, *lw["ff1"][1], lw["ff2"][1], [(y, vy)])
    ga, be = lw["styl"][4]
    sc, sh = m.ss_rows(c.st[:y.shape[0]], l, 4)
    t, vt = _lnv(y, vy, (ga * (1 + sc), be * (1 + sc) + sh))          # the pre-activation LN(y) (1 + scale) + shift
    s = t * torch.sigmoid(t)
    vs = _r16v(s, 1.1 ** 2 * vt + ((2 * UE + 4 * U) * s.abs()) ** 2)   # SiLU: slope <= 1.1; exp2 and a fast reciprocal
    out, vout = _mmv(s, vs, lw["ffo"][0], [(X3, None), (lw["ffo"][1], None)])
    return out, STAT * torch.sqrt(vout)


def seq_head_ref(m, X4):
    w, b = m.head
    return _lin(bf16(X4).double(), None, w, [b])


def where_worst(got, ref, bound, B=None):
    """The element with the worst |err| / bound of a [R, T, 512] stage, spelled out: sequence (kind and clip where B, the
    number of clips, is given), token block, wave."""
    r = (got.double() - ref).abs() / bound.clamp_min(1e-300)
    r = torch.where(got.double() == ref, torch.zeros_like(r), torch.nan_to_num(r, nan=float("inf")))
    i = int(r.reshape(-1).argmax())
    T = got.shape[1]
    s, t, f = i // (T * DM), (i // DM) % T, i % DM
    bad = (r > 1).nonzero()
    waves = sorted(set((bad[:, 2] // 64).tolist())) if len(bad) else []
    kind = "" if B is None else " (%s, clip %d)" % ("conditional" if s < B else "classifier-free", s % B)
    return ("worst %.3g at sequence %d%s token %d (block %d) feature %d (wave %d): got %.6g ref %.6g bound %.3g; %d elements "
            "over, in waves %s" % (float(r.reshape(-1)[i]), s, kind, t, t // 16, f, f // 64, float(got[s, t, f]),
                                   float(ref[s, t, f]), float(bound[s, t, f]), len(bad), waves))


# ---- fp32 / bf16 emulations in the kernels' operation order
_F = torch.float32


def _f(x):
    return x.float()


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _stats32(x):
    inv = torch.tensor(1.0 / DM, dtype=_F)
    mu = x.sum(-1, keepdim=True) * inv
    var = _fma(-mu, mu, (x * x).sum(-1, keepdim=True) * inv).clamp_min(0.0)
    return mu, torch.rsqrt(var + torch.tensor(1e-5, dtype=_F))


def _xhat32(x):
    mu, r = _stats32(x)
    return _fma(x, r, -mu * r), mu, r


def _mm(a, w):
    return bf16(a) @ _f(w).T


def _exp2sub(q, mx):
    l2 = torch.tensor(LOG2E, dtype=_F)
    return torch.exp2(_fma(q, l2, mx * -l2))


def _silu32(v):
    return v * (1.0 / (1.0 + torch.exp2(v * torch.tensor(-LOG2E, dtype=_F))))


def _gelu32(v):
    """rg_gelu_erf, operation for operation."""
    x = v.abs() * torch.tensor(0.70710678118654752440, dtype=_F)
    p = _fma(torch.tensor(1.904678831e-05, dtype=_F), x, torch.tensor(-4.679475024e-04, dtype=_F))
    for k in (5.123828382e-03, -3.364521737e-02, 1.520822882e-01, 9.172845077e-01, 1.628025418e+00):
        p = _fma(p, x, torch.tensor(k, dtype=_F))
    p = _fma(p, -x, torch.tensor(-1.0, dtype=_F))
    return _fma(-v.abs(), torch.exp2(p), v.clamp_min(0.0))


def _softmax32_emu(q):
    s = q.reshape(*q.shape[:-1], q.shape[-1] // HD, HD)
    e = _exp2sub(s, s.max(-1, keepdim=True).values)
    return (e * (1.0 / e.sum(-1, keepdim=True))).reshape(q.shape)


def _styl32(m, c, l, bi, y, n, all_step=False):
    """write_styl: the stylized bf16 panel of y [n sequences, T, 512] with the fp32 gain / offset the host folds per step."""
    ga, be = (_f(t) for t in m.layers[l]["styl"][bi])
    st = torch.full_like(c.st[:n], c.step) if all_step else c.st[:n]
    t = _f(m.ss[st, l, bi])
    sc1 = 1.0 + t[:, None, :DM]
    gain, off = ga * sc1, be * sc1 + t[:, None, DM:]
    xh, _, _ = _xhat32(y)
    return _silu32(_fma(xh, gain, off))


def seq_stage_emulate(stage, m, c, l, inp, mutant=None):
    """fp32 / bf16 emulation of one stage in the kernel's operation order, from the same inputs as its reference: stage 1 (inp:
    nothing), 10 (X), 2 (X, y), 11-13 (X: the state at stage 2), 3 (X, y3), 4 (X), 0 = the head (X).  mutant: a key of
    SEQ_MUTANTS, a deliberately wrong variant (it changes the stage it belongs to and no other)."""
    assert mutant is None or mutant in SEQ_MUTANTS
    B, T, H = c.B, c.T, DM // HD
    lw = m.layers[l] if stage else None
    if stage == 1:
        w, b = m.embed
        out = (_f(m.tbias)[None] + _f(b)) + _mm(c.x, w)
        return torch.cat([out, out])
    if stage == 0:
        w, b = m.head
        return _f(b) + _mm(inp["X"], w)
    X = _f(inp["X"])
    R = X.shape[0]
    if stage == 10:
        a = _xhat32(X)[0]
        k, v, q = (_f(lw[n][1]) + _mm(a, lw[n][0]) for n in ("k", "v", "q"))
        valid = (c.src_mask != 0)
        if mutant == "masked_token":
            valid = valid.clone()
            valid[:, (T - 3) // 4] = True
        if mutant == "pad_rows":                 # rows T .. 47 repeat token T - 1
            pad = 48 - T
            k, v = (torch.cat([t, t[:, -1:].expand(R, pad, DM)], 1) for t in (k, v))
            valid = torch.cat([valid, torch.ones(R, pad, dtype=torch.bool)], 1)
        k4, v4, vm = k.view(R, -1, H, HD), v.view(R, -1, H, HD), valid[:, :, None, None]
        mx = torch.where(vm, k4, torch.full_like(k4, -float("inf"))).max(dim=1, keepdim=True).values
        ex = torch.where(vm, _exp2sub(k4, torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))), torch.zeros_like(k4))
        s = ex.sum(dim=1, keepdim=True)
        P = ex * torch.where(s > 0, 1.0 / s, torch.zeros_like(s))
        A = torch.einsum("rthd,rthl->rhdl", bf16(P), bf16(v4))
        Q = bf16(_softmax32_emu(q)).view(R, T, H, HD)
        return torch.einsum("rthd,rhdl->rthl", Q, bf16(A)).reshape(R, T, DM)
    if stage == 2:
        w, b = lw["sao"]
        b = _f(b).clone()
        if mutant == "bias_wave1":
            b[64:128] = 0
        return (X + b) + _mm(_styl32(m, c, l, 0, _f(inp["y"]), R, mutant == "styl_step"), w)
    if stage in (11, 12, 13):
        cond = stage - 11
        q = _f(lw["q3"][cond][1]) + _mm(_xhat32(X)[0], lw["q3"][cond][0])
        Q = bf16(_softmax32_emu(q)).view(B, T, H, HD)
        A = bf16(c.A[l, cond])
        if mutant == "a_blocks_swapped" and cond == SEQ_MUTANTS[mutant] - 11:
            A = A.clone()
            A[:, 5] = torch.cat([A[:, 5, :, 16:], A[:, 5, :, :16]], -1)
        y = torch.einsum("rthd,rhdl->rthl", Q, A).reshape(B, T, DM)
        if not (mutant == "no_grid" and cond == SEQ_MUTANTS[mutant] - 11):
            z = y + torch.tensor(-1000000.0)
            y = torch.where((c.qm[cond] == 0)[:, :, None], z + torch.tensor(1000000.0), y)
        return y
    if stage == 3:
        xh, mu, r = _xhat32(X)
        c1 = _f(lw["wx32"].sum(1)) if mutant == "rowsum_fp32" else _f(lw["c1"])
        v = (c1 * mu + _f(lw["b_mix"])) * r + _mm(xh, lw["wx"])
        v = v * (1.0 / r)
        for cond in range(3):
            v[:B] += _mm(_styl32(m, c, l, 1 + cond, _f(inp["y3"][cond]), B), lw["mix"][cond])
            bv = _f(lw["bv"][cond])
            yu = torch.stack([bv, (bv + torch.tensor(-1000000.0)) + torch.tensor(1000000.0)])
            ga, be = (_f(t) for t in lw["styl"][1 + cond])
            t = _f(m.ss[c.st[B:], l, 1 + cond])
            sc1 = 1.0 + t[:, None, :DM]
            tab = bf16(_silu32(_fma(_xhat32(yu)[0][None], ga * sc1, be * sc1 + t[:, None, DM:])))      # [B, 2, 512]
            rows = (tab.double() @ lw["mix"][cond].T).float()
            flag = (c.qm[cond] == 0).long()
            if mutant == "unc_flag" and cond == 0:
                flag = flag.clone()
                flag[:, 1] = 1 - flag[:, 1]
            v[B:] += torch.gather(rows, 1, flag[:, :, None].expand(B, T, DM))
        return v
    if stage == 4:
        a = X
        yf = torch.zeros_like(X)
        for j in range(2):
            b1 = _f(lw["ff1"][j][1]).clone()
            if mutant == "ff1_bias_wave1" and j == 0:
                b1[64:128] = 0
            h = b1 + _mm(a, lw["ff1"][j][0])
            gg = _gelu32(h)
            if j == 0 or mutant == "ff2_bias_twice":
                yf = yf + _f(lw["b_ff2"])
            yf = yf + _mm(gg, lw["ff2"][j])
        w, b = lw["ffo"]
        b = _f(b).clone()
        if mutant == "ffo_bias_wave1":
            b[64:128] = 0
        if mutant == "ffo_bias_none":
            b[:] = 0
        return (X + b) + _mm(_styl32(m, c, l, 4, yf, R, mutant == "ffn_styl_step"), w)
    raise ValueError(stage)


def seq_stage_ref(stage, m, c, l, inp):
    """(ref, bound[, tie]) of a stage from the inputs `seq_stage_emulate` takes."""
    X = inp["X"].double() if "X" in inp else None
    if stage == 1:
        return seq_embed_ref(m, c)
    if stage == 0:
        return seq_head_ref(m, X)
    if stage == 10:
        return seq_sa_y_ref(m, c, l, X)
    if stage == 2:
        return seq_sa_out_ref(m, c, l, X, inp["y"].double())
    if stage in (11, 12, 13):
        return seq_ca_y_ref(m, c, l, stage - 11, X)
    if stage == 3:
        return seq_mix_ref(m, c, l, X, [y.double() for y in inp["y3"]])
    if stage == 4:
        return seq_ffn_ref(m, c, l, X)
    raise ValueError(stage)


def seq_stage_inputs(stage, c, state):
    """The teacher-forcing inputs of a stage out of `state`: dict stage -> tensor of the current layer (1 / 4: the state the
    layer starts from under key "in"; 11-13: [B, T, 512])."""
    B = c.B
    if stage == 10:
        return dict(X=state["in"])
    if stage == 2:
        return dict(X=state["in"], y=state[10])
    if stage in (11, 12, 13):
        return dict(X=state[2][:B])
    if stage == 3:
        return dict(X=state[2], y3=[state[11], state[12], state[13]])
    if stage == 4:
        return dict(X=state[3])
    raise ValueError(stage)


def adaln_table(g, L, timesteps):
    """ss [S, L, 5, 2 D] fp32: emb_layers(SiLU(time_embed(sinusoid(t)))) of every stylization block (diffusion_transformer.py:27-46,
    stylization_block.py:29-35), in fp64 on the CPU.  The GPU tests take the model's own table; this one feeds the CPU tests."""
    d = lambda n: g(n).double()
    half = DM // 2
    freqs = torch.exp(-np.log(10000.0) * torch.arange(half, dtype=F64) / half)
    args = torch.tensor(list(timesteps), dtype=F64)[:, None] * freqs[None]
    silu = lambda x: x * torch.sigmoid(x)
    emb = silu(torch.cat([torch.cos(args), torch.sin(args)], -1) @ d("time_embed.0.weight").T + d("time_embed.0.bias"))
    emb = silu(emb @ d("time_embed.2.weight").T + d("time_embed.2.bias"))
    blocks = ("sa_block", "ca_blocks.xf_text", "ca_blocks.xf_audio", "ca_blocks.xf_spk", "ffn")
    ss = torch.empty(len(timesteps), L, 5, 2 * DM, dtype=F64)
    for l in range(L):
        for bi, blk in enumerate(blocks):
            q = "temporal_decoder_blocks.%d.%s.proj_out.emb_layers.1." % (l, blk)
            ss[:, l, bi] = emb @ d(q + "weight").T + d(q + "bias")
    return ss.float()


# The launches of tests/test_seq_stages_gpu.py: (B, T, step, step_b, split); the CPU tests run the B = 1 ones.
SEQ_LAUNCHES = [(B, T, *s) for B in (1, 3) for T in (15, 27, 43, 47) for s in ((49, None, None), (0, None, None), (40, 9, 1))]


def seq_launch_case(B, T, step, step_b, split):
    return seq_case(B, T, 5000 + 100 * T + 10 * B + (step % 7), step, step_b, split)


def seq_frames(T):
    """max_seq_len that gives T = 4 (max_seq_len / 15) + 3 token rows."""
    assert (T - 3) % 4 == 0
    return 15 * (T - 3) // 4


# ---- rg_venc_forward: one block of the skip-transformer encoder (detr_utils.py:101-152, :335-393 forward_post)
VENC_HEADS = 4


class VencModel:
    """fp64 parameters of an encoder stack of `num_layers` layers from the VAE's state dict (reference key names)."""

    def __init__(self, sd, num_layers, name="encoder", heads=VENC_HEADS):
        D = DM
        self.heads = heads
        d = lambda k: sd[k].detach().double()
        nl = num_layers + 1 if num_layers % 2 == 0 else num_layers
        nb = self.nb = (nl - 1) // 2
        scale = torch.tensor(1.0 / float(D // heads) ** 0.5, dtype=torch.float32)      # folded into Q in fp32, as the host does
        names = ([("%s.input_blocks.%d" % (name, i), None) for i in range(nb)] + [(name + ".middle_block", None)] +
                 [("%s.output_blocks.%d" % (name, i), "%s.linear_blocks.%d" % (name, i)) for i in range(nb)])
        self.blocks = []
        for blk, skip in names:
            wi, bi = sd[blk + ".self_attn.in_proj_weight"].float(), sd[blk + ".self_attn.in_proj_bias"].float()
            w1, w2 = d(blk + ".linear1.weight"), d(blk + ".linear2.weight")
            b = dict(q=(_wb(wi[:D] * scale), (bi[:D] * scale).double()), q_raw=(_wb(wi[:D]), bi[:D].double()),
                     k=(_wb(wi[D:2 * D]), bi[D:2 * D].double()), v=(_wb(wi[2 * D:]), bi[2 * D:].double()),
                     o=(_wb(d(blk + ".self_attn.out_proj.weight")), d(blk + ".self_attn.out_proj.bias")),
                     n1=(d(blk + ".norm1.weight"), d(blk + ".norm1.bias")), n2=(d(blk + ".norm2.weight"), d(blk + ".norm2.bias")),
                     ff1=[(_wb(w1[j * D:(j + 1) * D]), d(blk + ".linear1.bias")[j * D:(j + 1) * D]) for j in range(2)],
                     ff2=[_wb(w2[:, j * D:(j + 1) * D]) for j in range(2)], b_ff2=d(blk + ".linear2.bias"), skip=None)
            if skip is not None:
                ws = d(skip + ".weight")
                b["skip"] = (_wb(ws[:, :D]), _wb(ws[:, D:]), d(skip + ".bias"))
            self.blocks.append(b)
        self.norm = (d(name + ".norm.weight"), d(name + ".norm.bias"))

    def skip_of(self, b):
        """Index of the block whose output block b takes as its skip state (None for input and middle blocks)."""
        return 2 * self.nb - b if b > self.nb else None


def venc_block_ref(m, b, X, Xs=None):
    """The state behind block b from the state X [n, S, 512] in front of it (the kernel's dump, exact fp32) and, for an output
    block, the skip state Xs.  Returns (out, bound): STAT standard deviations of the first-order variance model (module docstring,
    "statistical tier": eight chained roundings between two dumps leave a worst-case bound above the signal)."""
    blk = m.blocks[b]
    n, S = X.shape[:2]
    H, hd = m.heads, DM // m.heads
    X = X.double()
    if blk["skip"] is not None:
        wx, wsk, bs = blk["skip"]
        x, vx = _mmv(bf16(X).double(), None, wx, [(bs, None)])
        x, vx = _mmv(bf16(Xs).double(), None, wsk, [(x, vx)])
        a, va = x, _r16v(x, vx)
    else:
        x, vx, a, va = X, torch.zeros_like(X), bf16(X).double(), None
    q, k, v = (_mmv(a, va, blk[nm][0], [(blk[nm][1], None)]) for nm in ("q", "k", "v"))
    (q, vq), (k, vk), (v, vv) = ((t.view(n, S, H, hd), _r16v(t, tv).view(n, S, H, hd)) for t, tv in (q, k, v))
    qk = lambda q_, k_: torch.einsum("nihd,njhd->nhij", q_, k_)
    s = qk(q, k)
    vs = qk(vq, k * k) + qk(q * q, vk) + hd * (U * qk(q.abs(), k.abs())) ** 2
    P = torch.softmax(s, dim=-1)
    spread = (s.max(-1, keepdim=True).values - s.min(-1, keepdim=True).values).clamp(max=88.0)
    vP = P * P * (vs + (P * P * vs).sum(-1, keepdim=True) + (2 * U * spread + (S + 4) * U + 2 * UE) ** 2 + US ** 2 / 3)      # P as bf16 hi + lo
    pv = lambda p_, v_: torch.einsum("nhij,njhd->nihd", p_, v_)
    o = pv(P, v).reshape(n, S, DM)
    vo = (pv(vP, v * v) + pv(P * P, vv) + 48 * (U * pv(P, v.abs())) ** 2).reshape(n, S, DM)
    x1, v1 = _lnv(*_mmv(o, _r16v(o, vo), blk["o"][0], [(x, vx), (blk["o"][1], None)]), blk["n1"])
    va1 = _r16v(x1, v1)
    y, vy = x1, v1
    for j in range(2):
        y, vy = _ffn_hidden_var(x1, va1, *blk["ff1"][j], blk["ff2"][j], [(y, vy)] + ([(blk["b_ff2"], None)] if j == 0 else []))
    out, vout = _lnv(y, vy, blk["n2"])
    return out, STAT * torch.sqrt(vout)


def venc_final_ref(m, X):
    """`out`: the encoder's final LayerNorm of the state behind the last block."""
    out, var = _lnv(X.double(), torch.zeros_like(X, dtype=F64), m.norm)
    return out, STAT * torch.sqrt(var)


def _ln32(x, gb):
    mu, r = _stats32(x)
    return _fma((x - mu) * r, _f(gb[0]), _f(gb[1]))


def venc_block_emulate(m, b, X, Xs=None, mutant=None):
    """fp32 / bf16 emulation of one block in the kernel's operation order.  mutant: one of VENC_MUTANTS."""
    assert mutant is None or mutant in VENC_MUTANTS
    blk = m.blocks[b]
    n, S = X.shape[:2]
    H, hd = m.heads, DM // m.heads
    x = _f(X)
    if blk["skip"] is not None:
        wx, wsk, bs = blk["skip"]
        if mutant == "skip_swapped":
            wx, wsk = wsk, wx
        x = (_f(bs) + _mm(x, wx)) + _mm(_f(Xs), wsk)
    wq = blk["q_raw" if mutant == "no_scale" else "q"]
    q, k, v = (bf16(_f(w[1]) + _mm(x, w[0])).view(n, S, H, hd) for w in (wq, blk["k"], blk["v"]))
    s = torch.einsum("nihd,njhd->nhij", q, k)
    e = _exp2sub(s, s.max(-1, keepdim=True).values)
    P = e * (1.0 / e.sum(-1, keepdim=True))
    ph, pl = split_hi_lo(P)
    o = (torch.einsum("nhij,njhd->nihd", pl, v) + torch.einsum("nhij,njhd->nihd", ph, v)).reshape(n, S, DM)
    x = _ln32((x + _f(blk["o"][1])) + _mm(o, blk["o"][0]), blk["n2" if mutant == "norm2_for_norm1" else "n1"])
    y = x
    for j in range(2):
        gg = _gelu32(_f(blk["ff1"][j][1]) + _mm(x, blk["ff1"][j][0]))
        if j == 0:
            y = y + _f(blk["b_ff2"])
        y = y + _mm(gg, blk["ff2"][j])
    return _ln32(y, blk["n2"])


def venc_final_emulate(m, X):
    return _ln32(_f(X), m.norm)


VENC_SEED = 7


def venc_input(nseq, S, num_layers):
    """Embedded sequences [nseq, S, 512] of the size the encoder sees: unit-scale rows."""
    return randn((nseq, S, DM), 9000 + 100 * S + 10 * nseq + num_layers)


VENC_CASES = [(nl, S, nseq) for nl in (3, 5) for S in (2, 7, 16, 17, 24) for nseq in (1, 3)]


# ---- rg_vdec_step: one launch of the block-fused decoder (gesture_vae.py:195-239 `decode`; the same skip stack with pos =
# query_pos: q = k = x + pos, v = x, 32 heads of 16 over 160 tokens).  Module docstring, "Fused stacks": the decoder's tiers.
VDEC_HEADS = 32
VDEC_S = 160          # tokens of a sequence: four tiles of VDEC_TILE rows, one workgroup each
VDEC_TILE = 40
VDEC_MUTANTS = ("no_scale", "k_no_pos", "v_with_pos", "heads_of_32", "stale_tile", "drop_last_keys", "norm2_for_norm1",
                "skip_swapped", "no_final_norm")


def VdecModel(sd, num_layers):
    """The decoder stack's fp64 parameters (Q scaled by 1 / sqrt(16) = 0.25 in fp32) and `table`, the 160 rows of query_pos_decoder."""
    m = VencModel(sd, num_layers, name="decoder", heads=VDEC_HEADS)
    m.table = sd["query_pos_decoder.pe"][:VDEC_S, 0].detach().float().contiguous()
    return m


def _vdec_operands(x, pos):
    """The two bf16 operand panels of a launch's projections from the fp32 residual x and pos: (bf16(fp32(x + pos)), bf16(x))."""
    xf = x.float()
    return bf16(xf + pos.float()).double(), bf16(xf).double()


def vdec_skip_ref(m, b, X, Xs):
    """The residual in front of output block b: bias + bf16(X) Wx^T + bf16(Xs) Ws^T from the dumped states behind block b - 1 (X)
    and behind block skip_of(b) (Xs).  Worst-case tier: exact operands, one fp32 accumulation over 2 * 512 products and the two
    units' bias vectors (the second one zero)."""
    wx, wsk, bs = m.blocks[b]["skip"]
    a, s = bf16(X.float()).double(), bf16(Xs.float()).double()
    out = bs + a @ wx.T + s @ wsk.T
    mag = bs.abs() + a.abs() @ wx.abs().T + s.abs() @ wsk.abs().T
    return out, MARGIN * (2 * DM + 2) * U * mag


def vdec_proj_ref(m, b, x, pos):
    """Q, K, V of block b as fp32 values (before their bf16 stores) from the kernel's own fp32 residual x in front of the block's
    attention and the exact pos: {"q" / "k" / "v": (ref, bound)}.  Worst-case tier (`_lin`, exact operands); the stored bf16
    numbers go through `bf16_bounds`."""
    blk = m.blocks[b]
    xp, xb = _vdec_operands(x, pos)
    return {nm: _lin(a, None, blk[nm][0], [blk[nm][1]]) for nm, a in (("q", xp), ("k", xp), ("v", xb))}


def vdec_block_ref(m, b, x, pos):
    """The state behind block b from the fp32 residual x [n, 160, 512] in front of its attention (behind the skip linear of an
    output block: what a launch leaves in `x`) and pos.  Statistical tier, as `venc_block_ref`: 32 heads of 16, 160 keys in the
    softmax term, 2 * 160 roundings in the P V accumulation (hi and lo parts of P), x with variance 0 in the out_proj residual."""
    blk = m.blocks[b]
    n, S = x.shape[:2]
    H, hd = m.heads, DM // m.heads
    x = x.double()
    xp, xb = _vdec_operands(x, pos)
    q, k, v = (_mmv(a, None, blk[nm][0], [(blk[nm][1], None)]) for nm, a in (("q", xp), ("k", xp), ("v", xb)))
    (q, vq), (k, vk), (v, vv) = ((t.view(n, S, H, hd), _r16v(t, tv).view(n, S, H, hd)) for t, tv in (q, k, v))
    qk = lambda q_, k_: torch.einsum("nihd,njhd->nhij", q_, k_)
    s = qk(q, k)
    vs = qk(vq, k * k) + qk(q * q, vk) + hd * (U * qk(q.abs(), k.abs())) ** 2
    P = torch.softmax(s, dim=-1)
    spread = (s.max(-1, keepdim=True).values - s.min(-1, keepdim=True).values).clamp(max=88.0)
    vP = P * P * (vs + (P * P * vs).sum(-1, keepdim=True) + (2 * U * spread + (S + 4) * U + 2 * UE) ** 2 + US ** 2 / 3)      # P as bf16 hi + lo
    pv = lambda p_, v_: torch.einsum("nhij,njhd->nihd", p_, v_)
    o = pv(P, v).reshape(n, S, DM)
    vo = (pv(vP, v * v) + pv(P * P, vv) + 2 * S * (U * pv(P, v.abs())) ** 2).reshape(n, S, DM)
    x1, v1 = _lnv(*_mmv(o, _r16v(o, vo), blk["o"][0], [(x, None), (blk["o"][1], None)]), blk["n1"])
    va1 = _r16v(x1, v1)
    y, vy = x1, v1
    for j in range(2):
        y, vy = _ffn_hidden_var(x1, va1, *blk["ff1"][j], blk["ff2"][j], [(y, vy)] + ([(blk["b_ff2"], None)] if j == 0 else []))
    out, vout = _lnv(y, vy, blk["n2"])
    return out, STAT * torch.sqrt(vout)


def vdec_final_ref(m, X):
    """`x` after the last launch: the stack's final LayerNorm of the state behind the last block."""
    return venc_final_ref(m, X)


def vdec_block_emulate(m, b, X, pos, Xs=None, mutant=None, prev_kv=None):
    """fp32 / bf16 emulation of block b in the kernel's operation order, from the state X behind block b - 1 (the stack's input
    for b = 0), pos and, for an output block, the skip state Xs.  Returns a namespace: x (the residual behind the skip linear, X
    itself at input and middle blocks), q, k, v (the stored bf16 numbers, [n, 160, 512]) and out (the state behind the block).
    mutant: one of VDEC_MUTANTS; prev_kv: (k, v) of the previous block's emulation for "stale_tile" (None: zeros)."""
    assert mutant is None or mutant in VDEC_MUTANTS
    blk = m.blocks[b]
    n, S = X.shape[:2]
    H, hd = (m.heads // 2, 2 * DM // m.heads) if mutant == "heads_of_32" else (m.heads, DM // m.heads)
    x = _f(X)
    if blk["skip"] is not None:
        wx, wsk, bs = blk["skip"]
        if mutant == "skip_swapped":
            wx, wsk = wsk, wx
        x = (_f(bs) + _mm(x, wx)) + _mm(_f(Xs), wsk)
    xp = _f(pos) + x
    wq = blk["q_raw" if mutant == "no_scale" else "q"]
    q = bf16(_f(wq[1]) + _mm(xp, wq[0]))
    k = bf16(_f(blk["k"][1]) + _mm(x if mutant == "k_no_pos" else xp, blk["k"][0]))
    v = bf16(_f(blk["v"][1]) + _mm(xp if mutant == "v_with_pos" else x, blk["v"][0]))
    ka, va = k, v
    if mutant == "stale_tile":          # tile 1 of every sequence reads the other parity: the previous block's keys and values
        ka, va = k.clone(), v.clone()
        pk, pv_ = prev_kv if prev_kv is not None else (torch.zeros_like(k), torch.zeros_like(v))
        ka[:, VDEC_TILE:2 * VDEC_TILE], va[:, VDEC_TILE:2 * VDEC_TILE] = pk[:, VDEC_TILE:2 * VDEC_TILE], pv_[:, VDEC_TILE:2 * VDEC_TILE]
    elif mutant == "drop_last_keys":
        ka, va = k[:, :S - 16], v[:, :S - 16]
    Sk = ka.shape[1]
    s = torch.einsum("nihd,njhd->nhij", q.view(n, S, H, hd), ka.reshape(n, Sk, H, hd))
    e = _exp2sub(s, s.max(-1, keepdim=True).values)
    P = e * (1.0 / e.sum(-1, keepdim=True))
    ph, pl = split_hi_lo(P)
    vh = va.reshape(n, Sk, H, hd)
    o = (torch.einsum("nhij,njhd->nihd", pl, vh) + torch.einsum("nhij,njhd->nihd", ph, vh)).reshape(n, S, DM)
    x1 = _ln32((x + _f(blk["o"][1])) + _mm(o, blk["o"][0]), blk["n2" if mutant == "norm2_for_norm1" else "n1"])
    y = x1
    for j in range(2):
        gg = _gelu32(_f(blk["ff1"][j][1]) + _mm(x1, blk["ff1"][j][0]))
        if j == 0:
            y = y + _f(blk["b_ff2"])
        y = y + _mm(gg, blk["ff2"][j])
    return types.SimpleNamespace(x=x, q=q, k=k, v=v, out=_ln32(y, blk["n2"]))


def vdec_final_emulate(m, X, mutant=None):
    return _f(X) if mutant == "no_final_norm" else _ln32(_f(X), m.norm)


VDEC_SEED = 7
VDEC_CASES = [(nl, nseq) for nl in (3, 5) for nseq in (1, 3)]
VDEC_KINDS = ("latent", "dense")


def vdec_input(nseq, nl, kind):
    """The stack's input x [nseq, 160, 512] (pos = x + m.table, an fp32 add).  "latent": what the product feeds it, 10 unit-normal
    latent rows and 150 zero frame queries; "dense": every row a distinct unit-scale random row, so that exchanged rows, tiles or
    sequences show (zero rows are all alike)."""
    seed = 9500 + 10 * nseq + nl
    if kind == "dense":
        return randn((nseq, VDEC_S, DM), seed + 100)
    assert kind == "latent"
    return torch.cat((randn((nseq, 10, DM), seed), torch.zeros(nseq, VDEC_S - 10, DM)), dim=1)


def vdec_qimg_rows(img, ntiles):
    """A tile's Q panel image, int16 bit patterns of bf16 [ntiles][3 tb][16 s][4 gq][16 l][8 e], as rows: [ntiles, 48, 512] with
    Q[token 16 tb + l, feature 32 s + 8 gq + e] (rg_stationary.h: panel_store); rows >= 40 of a tile are padding."""
    return img.view(ntiles, 3, 16, 4, 16, 8).permute(0, 1, 4, 2, 3, 5).reshape(ntiles, 48, DM)
