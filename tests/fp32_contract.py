"""Inputs, fp64 references and derived per-element bounds of the plain-fp32 (vector ALU) kernels.

Shared by test_gpu_fp32_contract.py (the kernels on the GPU) and test_fp32_contract_bounds.py (the same
builders and bounds against fp32 CPU evaluations: the correct formula passes, deliberately wrong ones
fail).  Nothing here touches a device.

Every reference is torch fp64 written from the formula in include/spt_hip.h / the kernel's header
comment.  Every bound is first order in u = 2^-24 from the kernel's stated arithmetic, times SECOND
(1 + 2^-10) for the products of two error terms.  A sum's error is exact.fp32_tree_bound(sum of
|terms|, depth): the depth is the number of roundings a term passes through, read off the kernel's
summation structure and stated beside each use.  The ulp errors of the device functions are the only
figures that are not derived; they are the named constants below, with the rule that fixes them.

Inputs follow the contract tier: rows (or columns, or slices) scaled by 2^-12 .. 2^0 in a fixed cycle,
so that a known share of the elements is small against the tensor's maximum.
"""
import math

import torch

import exact as X

U = 2.0 ** -24
SECOND = 1 + 2.0 ** -10

def f32(x: float) -> float:
    """A Python float as the fp32 value a kernel receives for it."""
    return float(torch.tensor(x, dtype=torch.float32))


# Device function errors, in ulp of the result (u |value| each): the one part of a bound that cannot be
# derived from the source.  Each starts from the figure the kernel's own comment gives ("~2 ulp" for
# __expf / __logf in head_loss.hip, "1 ulp" for v_rcp_f32 in pq_loss.hip; 2 where there is none).  The rule
# for the figure that ships: run test_gpu_fp32_contract.py on the MI355X, read the "[function]" lines (the
# largest error against the fp64 reference with the structural part of the bound subtracted), take the
# smallest power of two >= 4 x the largest, 16 at the most.  Figures of the MI355X run in the comments.
RSQRT_ULPS = 4        # rsqrtf (v_rsq_f32): 0.68 ulp measured
EXPF_ULPS = 2         # expf, the precise one (softmax.hip, routing.hip, fused_attention.hip): 0.38 ulp measured (silu)
FAST_EXP_ULPS = 1     # __expf = v_exp_f32(x log2e), plus |x| u for the pre-scale (eval_bound's arg): nothing beyond
                      # the structural bound measured (<= 0)
FAST_LOG_ULPS = 1     # __logf = v_log_f32(x) ln2: nothing beyond the structural bound measured (<= 0)
DIV_ULPS = 1          # a / b, 1.0f / b: correctly rounded (built with -fno-fast-math)
LOG2E_REL = abs(f32(math.log2(math.e)) / math.log2(math.e) - 1)      # 1.3e-8: the constant of __expf's pre-scale


def row_exponents(n: int, step: int = 1) -> torch.Tensor:
    """[n] exponents 0 .. 12 in a fixed cycle: element i gets (i * step) % 13."""
    return (torch.arange(n) * step) % 13


def small_share(t: torch.Tensor) -> float:
    t = t.detach().double().abs()
    return float((t < 1e-3 * t.max()).double().mean())


def check(outputs: dict, refs: dict, what: str) -> dict:
    """assert_within for every output named in `refs` ({name: (ref64, bound)}); all are checked before
    the first failure is raised.  Returns {name: worst ratio}."""
    ratios, failures = {}, []
    for name, (ref, bound) in refs.items():
        try:
            ratios[name] = X.assert_within(outputs[name], ref, bound, '{} {}'.format(what, name))
        except AssertionError as e:
            failures.append(str(e))
    if failures:
        raise AssertionError('\n'.join(failures))
    return ratios


# ----------------------------------------------------------------------------------- norm kernels
#
# layernorm.hip.  A wave (or W waves, the wide rows) owns a row of d = 256 NV W floats.  A row sum:
# every lane adds NV float4 serially, each float4 first summed as (x + y) + (z + w): NV + 2 roundings;
# the 6-level butterfly; the W group partials added in order: W - 1.  row_depth = NV + 2 + 6 + W - 1.
# The sum is then multiplied by the fp32 constant 1 / d (its own rounding, and the product's): + 2.

def norm_form(d: int, rms: bool):
    """(NV, W) of layernorm.hip's spt_layernorm_form: 1 wave per row at d / 256 in {1, 2, 3, 4, 8}
    (RMS: also 16); d = 2560 -> (5, 2); LayerNorm 4096 -> (4, 4); 5120 -> (5, 4)."""
    if d in (256, 512, 768, 1024, 2048) or (d == 4096 and rms):
        return d // 256, 1
    return {2560: (5, 2), 4096: (4, 4), 5120: (5, 4)}[d]


def norm_partial_rows(rows: int) -> int:
    """spt_layernorm_partial_rows: one partial row per workgroup, min(ceil(rows / 8), 512)."""
    return min((rows + 7) // 8, 512)


def norm_row_depth(d: int, rms: bool) -> int:
    nv, w = norm_form(d, rms)
    return nv + 2 + 6 + (w - 1)


def norm_param_depth(d: int, rms: bool, rows: int) -> int:
    """dgamma / dbeta of a column: the rows one wave walks, one fma each; the 8 / W waves of a workgroup
    that hold the column, added in order; then layernorm_param_reduce_kernel over the partial rows: 16
    row lanes, each ceil(nparts / 16) rows in two alternating accumulators (ceil(nparts / 32)
    additions), a0 + a1, and the 16 lanes in order."""
    _, w = norm_form(d, rms)
    nparts = norm_partial_rows(rows)
    groups = nparts * (8 // w)
    walked = (rows + groups - 1) // groups
    return walked + (8 // w - 1) + (nparts + 31) // 32 + 1 + 16


def norm_inputs(d: int, rows: int, rms: bool, seed: int, add: bool = True):
    """x (+ r), gamma, beta, dy, dskip.  Row i: standard deviation 2^-(i % 13), mean up to 64 standard
    deviations, different per row (RMS: mean 0).  gamma / beta columns and dy rows and columns are
    scaled by 2^-12 .. 1 as well, so y, dx, dgamma and dbeta all have small elements."""
    gen = torch.Generator().manual_seed(seed)
    sigma = torch.pow(2.0, -row_exponents(rows).float())[:, None]      # (powers of two: exact scalings in fp32)
    mult = torch.zeros([rows, 1])
    if not rms:
        mult = (-64 + 128 * ((torch.arange(rows) * 11) % rows).float() / (rows - 1))[:, None]
    s0 = (torch.randn([rows, d], generator=gen) + mult) * sigma
    r = torch.randn([rows, d], generator=gen) * sigma if add else None
    x = s0 - r if add else s0
    col = torch.pow(2.0, -row_exponents(d, 5).float())
    gamma = (1 + 0.1 * torch.randn([d], generator=gen)) * col
    beta = None if rms else 0.1 * torch.randn([d], generator=gen) * col
    dy = torch.randn([rows, d], generator=gen) * torch.pow(2.0, -row_exponents(rows, 3).float())[:, None] \
        * torch.pow(2.0, -row_exponents(d, 7).float())
    dskip = torch.randn([rows, d], generator=gen) * sigma if add else None
    return dict(x=x, r=r, gamma=gamma, beta=beta, dy=dy, dskip=dskip, eps=1e-5)


def norm_forward_refs(inp, rms: bool, rsqrt=RSQRT_ULPS, only_rstd: bool = False):
    """{s, mean, rstd, y}: (fp64 reference, bound).

    s = fl(x + r): one fp32 addition, the same on every IEEE machine: exact (bound 0).
    mean = sum(s) / d:  tree_bound(sum |s| / d, row_depth + 2).
    var: with a_i = fl(s_i - mean^) (one rounding of a_i: 2 u of a_i^2), the square's rounding, the tree
      and the 1 / d: tree_bound(., row_depth + 5) of sum (s_i - mean^)^2 / d, which is var + dmean^2
      exactly (sum (s_i - mean) = 0); then + eps, one rounding of var + eps.
    rstd = rsqrtf(var + eps): half the relative error of its argument, plus the function's RSQRT_ULPS.
    y = fma(fl(fl(s - mean^) rstd^), gamma, beta): the mean's error moves (s - mean) by dmean, the
      subtraction and the product round (s - mean) rstd twice, rstd's error is relative to it, and
      the fma rounds y once."""
    x, r, gamma, beta, eps = inp['x'], inp['r'], inp['gamma'], inp['beta'], inp['eps']
    d = x.size(-1)
    depth = norm_row_depth(d, rms)
    s32 = x + r if r is not None else x
    s = s32.double()
    refs = {}
    if r is not None:
        refs['s'] = (s, torch.zeros(()))
    if rms:
        mean, dmean = torch.zeros(s.size(0), dtype=torch.float64), torch.zeros(s.size(0), dtype=torch.float64)
    else:
        mean = s.mean(-1)
        dmean = X.fp32_tree_bound(s.abs().mean(-1), depth + 2)
        refs['mean'] = (mean, dmean)
    c = s - mean[:, None]
    var = c.square().mean(-1)
    v = var + f32(eps)
    dv = X.fp32_tree_bound(var + dmean ** 2, depth + 5) + dmean ** 2 + U * v
    rstd = v.rsqrt()
    drstd = (0.5 * dv / v * rstd + X.eval_bound(rstd, rsqrt)) * SECOND
    refs['rstd'] = (rstd, drstd)
    if only_rstd:
        return refs
    g = gamma.double()
    y = c * rstd[:, None] * g
    dy_ = g.abs() * (rstd[:, None] * dmean[:, None] + c.abs() * (2 * U * rstd + drstd)[:, None])
    if beta is not None:
        y = y + beta.double()
    refs['y'] = (y, (dy_ + U * y.abs()) * SECOND)
    return refs


def norm_backward_refs(inp, s32, mean32, rstd32, rms: bool):
    """{dx, dgamma, dbeta} on the s, mean and rstd the backward is GIVEN (the forward's stored fp32).

    xhat^ = fl(fl(s - mean) rstd): 2 u.  g^ = fl(dy gamma): u.
    c1 = mean(g): tree_bound(mean |g|, row_depth + 3)  (g's rounding, the tree, the 1 / d)
    c2 = mean(g xhat): tree_bound(mean |g xhat|, row_depth + 6)  (g 1, xhat 2, the product 1)
    dx = fl(rstd fl(fl(g - c1) - fl(xhat c2))) (+ dskip):
      rstd (dc1 + |xhat| dc2 + u (|g| + 3 |xhat c2| + |g - c1| + |g - c1 - xhat c2|)) + u |dx| (+ u |dx + dskip|)
    dgamma = sum_rows dy xhat: xhat's 2 roundings and norm_param_depth; dbeta = sum_rows dy:
      norm_param_depth.  RMS: mean 0, c1 0, dbeta exactly 0."""
    gamma, dy32, dskip = inp['gamma'], inp['dy'], inp['dskip']
    rows, d = s32.shape
    depth = norm_row_depth(d, rms)
    s, dy, rstd = s32.double(), dy32.double(), rstd32.double()[:, None]
    mean = torch.zeros([rows, 1], dtype=torch.float64) if rms else mean32.double()[:, None]
    xh = (s - mean) * rstd
    g = dy * gamma.double()
    if rms:
        c1, dc1 = torch.zeros([rows, 1], dtype=torch.float64), torch.zeros([rows, 1], dtype=torch.float64)
    else:
        c1 = g.mean(-1, keepdim=True)
        dc1 = X.fp32_tree_bound(g.abs().mean(-1, keepdim=True), depth + 3)
    c2 = (g * xh).mean(-1, keepdim=True)
    dc2 = X.fp32_tree_bound((g * xh).abs().mean(-1, keepdim=True), depth + 6)
    t = g - c1 - xh * c2
    dx = rstd * t
    bound = rstd * (dc1 + xh.abs() * dc2 + U * (g.abs() + 3 * (xh * c2).abs() + (g - c1).abs() + t.abs())) \
        + U * dx.abs()
    if dskip is not None:
        dx = dx + dskip.double()
        bound = bound + U * dx.abs()
    pdepth = norm_param_depth(d, rms, rows)
    refs = {'dx': (dx, bound * SECOND),
            'dgamma': ((dy * xh).sum(0), X.fp32_tree_bound((dy * xh).abs().sum(0), pdepth + 2) * SECOND)}
    refs['dbeta'] = (torch.zeros(d, dtype=torch.float64), torch.zeros(())) if rms else \
        (dy.sum(0), X.fp32_tree_bound(dy.abs().sum(0), pdepth))
    return refs


# -------------------------------------------------------------------------------------- head loss
#
# head_loss.hip: a workgroup of 256 threads owns a row of ld / 4 float4.  mx is the exact maximum.
# e_i = __expf(fl(z_i - mx)): the subtraction rounds the argument (|a| u of e), the pre-scale another
# |a| u, the fp32 constant log2e it multiplies by is off by LOG2E_REL (|a| LOG2E_REL of e, one-sided), the
# function FAST_EXP_ULPS.  sum: a thread adds ceil(ld / 1024) float4 serially, each summed as
# (x + y) + (z + w): + 2; 6 butterfly levels; the four waves as (a + b) + (c + d): + 2.
# loss = fl(fl(__logf(sum) + mx) - z_t);  w = fl(scale / sum);  grad_i = fl(e_i w) (- scale at the target).

def head_loss_inputs(V: int, ld: int, seed: int, rows: int = 33):
    """Logit rows with spread (max - min) 1 .. 40, row by row, at offsets up to +-20; every 4th target
    ignored; pad columns hold a finite value the kernel must not read into the result."""
    gen = torch.Generator().manual_seed(seed)
    spread = (1 + 39 * torch.arange(rows).double() / (rows - 1))[:, None]
    z = torch.rand([rows, V], generator=gen, dtype=torch.float64)
    z[:, 0], z[:, V - 1] = 0.0, 1.0                                   # the spread is reached
    z = z * spread + 40 * (torch.rand([rows, 1], generator=gen, dtype=torch.float64) - 0.5)
    logits = torch.full([rows, ld], 7.0)
    logits[:, :V] = z.float()
    target = torch.randint(0, V, [rows], generator=gen)
    target[::4] = -100
    counted = int((target >= 0).sum())
    return dict(logits=logits, V=V, target=target, scale=torch.tensor([1.0 / counted]))


def head_loss_refs(inp, fast_exp=FAST_EXP_ULPS, fast_log=FAST_LOG_ULPS):
    logits, V, target = inp['logits'], inp['V'], inp['target']
    rows, ld = logits.shape
    scale = inp['scale'].double().item()
    z = logits[:, :V].double()
    counted = target >= 0
    mx = z.max(-1, keepdim=True).values
    a = z - mx
    e = a.exp()
    de = X.eval_bound(e, fast_exp, arg=a) + a.abs() * (U + LOG2E_REL) * e
    total = e.sum(-1, keepdim=True)
    depth = (ld // 4 + 255) // 256 + 2 + 6 + 2
    dtotal = X.fp32_tree_bound(total, depth) + de.sum(-1, keepdim=True)
    zt = z.gather(1, target.clamp_min(0)[:, None])
    lse = total.log()
    loss = (lse + mx - zt)[:, 0]
    dloss = (dtotal / total + X.eval_bound(lse, fast_log) + U * (lse + mx).abs())[:, 0] + U * loss.abs()
    w = scale / total
    dw = w * (dtotal / total + DIV_ULPS * U)
    grad = e * w
    onehot = torch.zeros_like(grad).scatter_(1, target.clamp_min(0)[:, None], 1.0)
    dgrad = w * de + e * dw + U * grad
    grad = grad - onehot * scale
    dgrad = (dgrad + U * onehot * grad.abs()) * SECOND
    full, dfull = torch.zeros([rows, ld], dtype=torch.float64), torch.zeros([rows, ld], dtype=torch.float64)
    full[:, :V] = grad * counted[:, None]              # ignored rows, pad columns: exactly 0
    dfull[:, :V] = dgrad * counted[:, None]
    return {'loss': (loss * counted, dloss * SECOND * counted), 'grad': (full, dfull)}


# ---------------------------------------------------------------------------------- sparse softmax
#
# softmax.hip: G consecutive lanes own a CSR row; G = pow2_ceil((nnz / S + 3) / 4) in [4, 64].  Row
# bounds and nnz all multiples of 4: a lane adds 4 values per step of 4 G, serially; else one per step
# of G.  Then log2 G butterfly levels.  No max subtraction; the denominator is max(1e-9f, sum), the
# backward's c = max(1e-9f, sum mask y dy): max is 1-Lipschitz, so the floor needs no exclusion.

def softmax_group(nnz: int, S: int) -> int:
    g = 1
    while g < (nnz // S + 3) // 4:
        g *= 2
    return min(max(g, 4), 64)


def softmax_depth(indptr: torch.Tensor, nnz: int, S: int) -> torch.Tensor:
    """[S] roundings a term of each row's sum passes through."""
    G = softmax_group(nnz, S)
    start, end = indptr[:-1].long(), indptr[1:].long()
    length = end - start
    vec = ((start | end | nnz) & 3) == 0
    serial = torch.where(vec, 4 * ((length + 4 * G - 1) // (4 * G)), (length + G - 1) // G)
    return serial + int(math.log2(G))


def softmax_inputs(kind: str, causal: bool, seed: int, B: int = 3, S: int = 96):
    """kind: 'z16' / 'z64' (uniform rows) or 'ragged' (row starts that are no multiples of 4, empty rows).
    causal: every column <= its row (duplicates of column 0 fill short rows); else columns anywhere in
    [0, S): those > row are masked, and rows whose columns are all masked sum to 0, under the floor.
    Scores in [-10, 10]; three rows per slice in [-30, -25]: their sums fall under the 1e-9 floor."""
    gen = torch.Generator().manual_seed(seed)
    if kind == 'ragged':
        length = torch.randint(0, 40, [S], generator=gen)
        length[5], length[6], length[0] = 0, 0, 3
    else:
        length = torch.full([S], int(kind[1:]))
    indptr = torch.cat([torch.zeros(1, dtype=torch.long), length.cumsum(0)]).int()
    nnz = int(indptr[-1])
    row_of = torch.repeat_interleave(torch.arange(S), length)
    cols = torch.randint(0, S, [B, nnz], generator=gen)
    if causal:
        cols = cols % (row_of + 1)
    values = 20 * torch.rand([B, nnz], generator=gen, dtype=torch.float64) - 10
    low = torch.isin(row_of, torch.tensor([7, 40, S - 1]))
    values = torch.where(low, -30 + 5 * torch.rand([B, nnz], generator=gen, dtype=torch.float64), values)
    dy = torch.randn([B, nnz], generator=gen, dtype=torch.float64) \
        * torch.pow(2.0, -row_exponents(S).double())[row_of]
    return dict(indptr=indptr, indices=cols.int(), values=values.float(), dy=dy.float(), row_of=row_of, S=S,
                nnz=nnz, scale=0.125, clamp=10.0)


FLOOR32 = float(torch.tensor(1e-9, dtype=torch.float32))


def _row_sums(t, row_of, S):
    return torch.zeros([t.size(0), S], dtype=torch.float64).index_add_(1, row_of, t)


def softmax_forward_refs(inp, expf=EXPF_ULPS):
    """y_p = mask_p exp(v_p) / max(1e-9, sum_row mask exp(v)): e's EXPF_ULPS; the sum's tree over the
    row and sum de; 1.0f / sum (DIV_ULPS) and the product, one rounding each."""
    row_of, S, nnz = inp['row_of'], inp['S'], inp['nnz']
    mask = (inp['indices'].long() <= row_of).double()
    e = mask * inp['values'].double().exp()
    de = X.eval_bound(e, expf)
    depth = softmax_depth(inp['indptr'], nnz, S).double()
    total = _row_sums(e, row_of, S)
    dtotal = depth * U / (1 - depth * U) * total + _row_sums(de, row_of, S)       # gamma_depth, depth per row
    den = total.clamp_min(FLOOR32)
    y = e / den[:, row_of]
    dy_ = y * (dtotal / den)[:, row_of] + de / den[:, row_of] + (DIV_ULPS + 1) * U * y
    return {'y': (y, dy_ * SECOND)}


def softmax_backward_refs(inp, y32, clamped=None):
    """grad_p = mask_p y_p (dy_p - c), c = max(1e-9, sum_row mask y dy), on the GIVEN y.  c: each product
    rounds once, then the row's tree.  (dy - c) rounds once, the product once.  Clamped form: times
    `scale` where |clamped_scores| < clamp (one more rounding), exactly 0 elsewhere."""
    row_of, S, nnz = inp['row_of'], inp['S'], inp['nnz']
    mask = (inp['indices'].long() <= row_of).double()
    y, dy = y32.double() * mask, inp['dy'].double()
    depth = softmax_depth(inp['indptr'], nnz, S).double() + 1
    c = _row_sums(y * dy, row_of, S)
    dc = (depth * U / (1 - depth * U) * _row_sums((y * dy).abs(), row_of, S))[:, row_of]
    c = c.clamp_min(FLOOR32)[:, row_of]
    grad = y * (dy - c)
    bound = y.abs() * (dc + U * (dy - c).abs()) + U * grad.abs()
    if clamped is not None:
        inside = (clamped.double().abs() < inp['clamp']).double()
        grad = grad * inp['scale'] * inside
        bound = (bound * inp['scale'] + U * grad.abs()) * inside
    return {'grad': (grad, bound * SECOND)}


def softmax_clamped_scores(inp):
    """clamp(values, -clamp, clamp) with every 5th entry moved onto a rail, exactly +-clamp."""
    c = inp['values'].clone().clamp(-inp['clamp'], inp['clamp'])
    flat = c.view(-1)
    flat[::5] = inp['clamp']
    flat[2::10] = -inp['clamp']
    return c


# -------------------------------------------------------------------- elementwise: swiglu, rotary
#
# routing.hip: silu(x) = x / (1 + expf(-x)).  e = expf(-x) (EXPF_ULPS of e), 1 + e rounds once, the
# division once: relative (EXPF_ULPS e / (1 + e) + 1 + DIV_ULPS) u =: r.  sigmoid sg = 1 / (1 + e): the same r.
# silu'(x) = sg (1 + x (1 - sg)): (1 - sg) has the ABSOLUTE error sg r + u (1 - sg); times |x| and a
# rounding; 1 + . cancels for x < 0, so its error stays absolute; then the product with sg.

def swiglu_inputs(rows: int, n: int, seed: int):
    """gate in [-30, 30]; side and dh rows scaled by 2^-12 .. 1."""
    gen = torch.Generator().manual_seed(seed)
    scale = torch.pow(2.0, -row_exponents(rows).double())[:, None]
    g = (60 * torch.rand([rows, n], generator=gen, dtype=torch.float64) - 30).float()
    g[0, :4] = torch.tensor([-30.0, 30.0, 0.0, -1.2784645])          # the ends, 0, silu's flat point
    s = (torch.randn([rows, n], generator=gen, dtype=torch.float64) * scale).float()
    dh = (torch.randn([rows, n], generator=gen, dtype=torch.float64) * scale).float()
    return dict(g=g, s=s, dh=dh)


def _sigmoid_parts(g, expf):
    e = (-g).exp()
    sg = 1 / (1 + e)
    r = (expf * e / (1 + e) + 1 + DIV_ULPS) * U
    return sg, r


def swiglu_forward_refs(inp, expf=EXPF_ULPS):
    g, s = inp['g'].double(), inp['s'].double()
    sg, r = _sigmoid_parts(g, expf)
    h = g * sg * s
    return {'h': (h, (r + U) * h.abs() * SECOND)}


def swiglu_backward_refs(inp, got_dg, got_ds, expf=EXPF_ULPS):
    """dg = fl(fl(dh s) silu'(g)), ds = fl(dh silu(g)); the row dots: <dh, h> from the kernel's own
    silu (its error r per term, the product a s, the fma), <dg, g> and <ds, s> of the STORED dg, ds: n / 256
    steps of 4 fmas per lane, then 6 butterfly levels."""
    g, s, dh = inp['g'].double(), inp['s'].double(), inp['dh'].double()
    n = g.size(1)
    sg, r = _sigmoid_parts(g, expf)
    inner = 1 + g * (1 - sg)
    dinner = g.abs() * (sg * r + 2 * U * (1 - sg)) + U * inner.abs()
    slope = sg * inner
    dslope = sg * dinner + slope.abs() * (r + U)
    dg = dh * s * slope
    ds = dh * g * sg
    depth = 4 * ((n + 255) // 256) + 6
    h = g * sg * s
    refs = {'dg': (dg, ((dh * s).abs() * dslope + 2 * U * dg.abs()) * SECOND),
            'ds': (ds, (r + U) * ds.abs() * SECOND),
            'dot_h': ((dh * h).sum(1), (X.fp32_tree_bound((dh * h).abs().sum(1), depth + 1)
                                        + (r * (dh * h).abs()).sum(1)) * SECOND)}
    for name, a, b in (('dot_g', got_dg, g), ('dot_s', got_ds, s)):
        a = a.detach().double().cpu()
        refs[name] = ((a * b).sum(1), X.fp32_tree_bound((a * b).abs().sum(1), depth))
    return refs


# rotary.hip: out = fl(fl(c x) -+ fl(s x')) (or one product and an fma): three roundings of the two
# products' magnitudes at most; the parts that are not rotated are copied: exact.

def rotary_inputs(n_parts: int, seed: int, N: int = 2, S: int = 125, H: int = 2, E: int = 24):
    """N S H = 500 rows of E / 8 = 3 float4 pairs: 1500 threads, no multiple of 256.  Rows scaled by 2^-12 .. 1;
    cos / sin tables of the positions at the usual frequencies, longer than S."""
    gen = torch.Generator().manual_seed(seed)
    parts = [(torch.randn([N, S, H, E], generator=gen, dtype=torch.float64)
              * torch.pow(2.0, -row_exponents(N * S * H).double()).view(N, S, H, 1)).float() for _ in range(n_parts)]
    freq = torch.pow(10000.0, -torch.arange(0, E, 2).double() / E)
    angle = torch.arange(S + 3).double()[:, None] * torch.cat([freq, freq])[None]
    return dict(parts=parts, cos=angle.cos().float(), sin=angle.sin().float())


def rotary_refs(inp, n_rot: int, transpose: bool):
    parts, cos, sin = inp['parts'], inp['cos'].double(), inp['sin'].double()
    N, S, H, E = parts[0].shape
    c, s = cos[:S].view(1, S, 1, E), sin[:S].view(1, S, 1, E)
    half = E // 2
    out, bound = [], []
    for p, x32 in enumerate(parts):
        x = x32.double()
        if p >= n_rot:
            out.append(x)
            bound.append(torch.zeros_like(x))
            continue
        lo, hi = x[..., :half], x[..., half:]
        if not transpose:              # y = cos x + sin rotate_half(x), rotate_half(x) = [-x_hi | x_lo]
            t1, t2 = c * x, s * torch.cat([-hi, lo], -1)
        else:                          # the adjoint: dx_lo = cos_lo dy_lo + sin_hi dy_hi, dx_hi = cos_hi dy_hi - sin_lo dy_lo
            t1, t2 = c * x, torch.cat([s[..., half:] * hi, -s[..., :half] * lo], -1)
        out.append(t1 + t2)
        bound.append(X.fp32_tree_bound(t1.abs() + t2.abs(), 2))
    return {'out': (torch.stack(out), torch.stack(bound))}


# ------------------------------------------------------------------------------ routing passes
#
# routing.hip.  The integer outputs (token, block, pos) are checked for what they must be -- the k
# largest of a token's values, sorted by block and then by token -- on inputs whose values in a row are
# further apart than the rounding of logit + bias (asserted by the builder): no selection is in doubt.

def route_inputs(T: int, G: int, seed: int):
    """prob [T, G] in (0, 1) with rows scaled by 2^-12 .. 1; logits [T, G] in [-20, 20] (in a wider
    matrix, as the kernel is given them) and a bias; distinct within every row."""
    gen = torch.Generator().manual_seed(seed)
    prob = (torch.rand([T, G], generator=gen, dtype=torch.float64)
            * torch.pow(2.0, -row_exponents(T).double())[:, None]).float()
    wide = torch.zeros([T, (G + 7) // 4 * 4])               # (row stride: a multiple of 4)
    wide[:, :G] = (40 * torch.rand([T, G], generator=gen, dtype=torch.float64) - 20).float()
    bias = (0.5 * torch.randn([G], generator=gen, dtype=torch.float64)).float()
    for rows in (prob.double(), wide[:, :G].double() + bias.double()):
        gaps = rows.sort(-1).values.diff(dim=-1)
        assert int((gaps <= 64 * U * rows.abs().max(-1, keepdim=True).values).sum()) == 0
    dcoeff = torch.randn([T * 2], generator=gen) * torch.pow(2.0, -row_exponents(T * 2).float())
    return dict(prob=prob, logits=wide, bias=bias, G=G, dcoeff=dcoeff, scale=f32(0.7))


def route_selection(values64: torch.Tensor, k: int):
    """(token, block, pos) of the counting sort: the k largest per token, by block, then by token."""
    T, G = values64.shape
    chosen = torch.zeros([T, G], dtype=torch.bool).scatter_(1, values64.topk(k, dim=-1).indices, True)
    block, token = chosen.t().nonzero(as_tuple=True)                  # block-major, tokens ascending
    place = torch.full([T, G], -1, dtype=torch.long)
    place[token, block] = torch.arange(T * k)
    pos = place[chosen].view(T, k)                                    # a token's blocks, ascending
    return token, block, pos


def route_prob_refs(inp, expf=EXPF_ULPS):
    """prob = 1 / (1 + expf(-(logit + bias))): the sigmoid's r of swiglu above, and the addition's
    rounding u |v| through the sigmoid's slope sg (1 - sg)."""
    G = inp['G']
    v = inp['logits'][:, :G].double() + inp['bias'].double()
    sg, r = _sigmoid_parts(v, expf)
    return sg, sg * (r + (1 - sg) * v.abs() * U) * SECOND


def route_backward_refs(inp, token, block, prob32=None):
    """d prob[t, g] = fl(scale dcoeff[p]) where row p is token t's selection of block g, 0 elsewhere; with
    `prob`: fl(fl(v fl(1 - y)) y): four roundings."""
    T, G = inp['prob'].shape
    out = torch.zeros([T, G], dtype=torch.float64)
    out[token, block] = inp['scale'] * inp['dcoeff'].double()
    if prob32 is None:
        return {'dprob': (out, U * out.abs())}
    y = prob32.double()
    out = out * (1 - y) * y
    return {'dlogit': (out, 4 * U * out.abs() * SECOND)}


def ffn_coeff_inputs(P: int, T: int, w: int, r: int, seed: int, floor: float = 1e-3):
    gen = torch.Generator().manual_seed(seed)
    scale = torch.pow(2.0, -row_exponents(P).double())[:, None]
    f = lambda *shape: torch.randn(list(shape), generator=gen, dtype=torch.float64)
    coeff = torch.rand([P], generator=gen) * 0.01                     # a tenth of them under the floor
    return dict(dot_main=(f(P, w) * scale).float(), dot_act=(f(P, w) * scale).float(), du=(f(P, r) * scale).float(),
                u=f(T, r).float(), dzt=f(T, r).float(), z=(f(P, r) * scale).float(),
                token=torch.randint(0, T, [P], generator=gen).int(), coeff=coeff, floor=floor)


def ffn_coeff_refs(inp):
    """out = (((sum dot_main + sum dot_act) - <du, u[token]>) - <dzt[token], z>) / max(coeff, floor): each
    sum of w terms a serial chain (w), then 3 more roundings; each dot r / 4 steps of a float4's products
    summed as (a + b) + (c + d): r / 4 + 3, then 2 (1) more; the division."""
    w, r = inp['dot_main'].size(1), inp['du'].size(1)
    tok = inp['token'].long()
    d1 = inp['du'].double() * inp['u'].double()[tok]
    d2 = inp['dzt'].double()[tok] * inp['z'].double()
    num = inp['dot_main'].double().sum(1) + inp['dot_act'].double().sum(1) - d1.sum(1) - d2.sum(1)
    dnum = X.fp32_tree_bound(inp['dot_main'].double().abs().sum(1) + inp['dot_act'].double().abs().sum(1), w + 3) \
        + X.fp32_tree_bound(d1.abs().sum(1), r // 4 + 5) + X.fp32_tree_bound(d2.abs().sum(1), r // 4 + 4)
    den = torch.maximum(inp['coeff'], torch.tensor(inp['floor'])).double()       # exact: a select of fp32 values
    out = num / den
    return {'out': (out, (dnum / den + DIV_ULPS * U * out.abs()) * SECOND)}


def embedding_inputs(T: int, width: int, n_rows: int, seed: int, repeats: int = 3000):
    """One id `repeats` times among T, the rest distinct; gradient rows scaled by 2^-12 .. 1."""
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randperm(n_rows - 1, generator=gen)[:T] + 1
    ids[torch.randperm(T, generator=gen)[:repeats]] = 0
    grad = (torch.randn([T, width], generator=gen, dtype=torch.float64)
            * torch.pow(2.0, -row_exponents(T).double())[:, None]).float()
    return dict(grad=grad, ids=ids, n_rows=n_rows)


def embedding_refs(inp):
    """Summed in fp64 (chunks of 64 positions, then the chunks), rounded to fp32 once: u |out|, and
    2^-50 sum |grad| for the fp64 additions."""
    g = inp['grad'].double()
    out = torch.zeros([inp['n_rows'], g.size(1)], dtype=torch.float64).index_add_(0, inp['ids'], g)
    mag = torch.zeros_like(out).index_add_(0, inp['ids'], g.abs())
    return {'out': (out, U * out.abs() + 2.0 ** -50 * mag)}


def combine_inputs(T: int, k: int, d: int, ns: int, seed: int):
    gen = torch.Generator().manual_seed(seed)
    f = lambda *shape: torch.randn(list(shape), generator=gen, dtype=torch.float64)
    rows = (f(T * k, d) * torch.pow(2.0, -row_exponents(T * k).double())[:, None]).float()
    side = (f(T, ns) * torch.pow(2.0, -row_exponents(T, 3).double())[:, None]).float()
    return dict(rows=rows, pos=torch.randperm(T * k, generator=gen).view(T, k).int(),
                bias=(0.01 * f(d)).float(), side=side, side_weight=f(ns, d).float())


def combine_refs(inp, with_side: bool):
    """out[t] = bias + sum_j rows[pos[t, j]] (+ sum_j side[t, j] side_weight[j]): one serial chain of k
    additions and ns fmas, from the bias on."""
    rows, pos = inp['rows'].double(), inp['pos'].long()
    out = inp['bias'].double() + rows[pos].sum(1)
    mag = inp['bias'].double().abs() + rows[pos].abs().sum(1)
    depth = pos.size(1)
    if with_side:
        out = out + inp['side'].double() @ inp['side_weight'].double()
        mag = mag + inp['side'].double().abs() @ inp['side_weight'].double().abs()
        depth += inp['side'].size(1)
    return {'out': (out, X.fp32_tree_bound(mag, depth))}


# ------------------------------------------------------------------- sddmm / spmm, gather forms
#
# sddmm.hip: out[b, p] = clamp(scale dot(q[b, row(p)], k[b, indices[b, p]])).  E = 64, 128 (gather4.h): a
# lane's 16 fmas, then log2(E / 16) butterfly levels; other E: 4 products / fmas per lane, then
# log2(pow2_ceil(E / 4)) levels.  One rounding for the scale; the clamp is exact and 1-Lipschitz.
# spmm.hip: y[b, r] = sum_{p in row r} values[b, p] x[b, indices[b, p]] (T: the roles of row and column
# exchanged, a sum over the entries of a COLUMN).  A sum of L entries, E = 64, 128: 16 fmas per 64-entry
# round in one lane, the four entry groups (+ 2), the wide mode's four slots (+ 3): 16 ceil(L / 64) + 5,
# and one addition per 512-row chunk in the chunked transposed form; other E: LPE = pow2_ceil(E / 4)
# fmas per round, then log2(64 / LPE) levels.

def sparse_inputs(B: int, S: int, E: int, kind: str, seed: int):
    """kind 'z16': what lookup produces -- 16 entries per row, columns <= row, short rows padded with
    duplicates of column 0; 'ragged': rows of 0 .. 39 entries (some empty), columns anywhere.  Rows of q,
    x and the values scaled by 2^-12 .. 1."""
    gen = torch.Generator().manual_seed(seed)
    if kind == 'ragged':
        length = torch.randint(0, 40, [S], generator=gen)
        length[3], length[S - 1] = 0, 0
    else:
        length = torch.full([S], int(kind[1:]))
    indptr = torch.cat([torch.zeros(1, dtype=torch.long), length.cumsum(0)]).int()
    nnz = int(indptr[-1])
    row_of = torch.repeat_interleave(torch.arange(S), length)
    cols = torch.randint(0, S, [B, nnz], generator=gen)
    if kind != 'ragged':
        slot = torch.arange(nnz) - indptr[:-1].long()[row_of]
        cols = torch.where(slot <= row_of, cols % (row_of + 1), torch.zeros_like(cols))
    f = lambda *shape: torch.randn(list(shape), generator=gen, dtype=torch.float64)
    rs = torch.pow(2.0, -row_exponents(S).double())
    return dict(indptr=indptr, indices=cols.int(), row_of=row_of, S=S, E=E, nnz=nnz,
                q=(f(B, S, E) * rs[:, None]).float(), k=f(B, S, E).float(),
                values=(f(B, nnz) * rs[row_of]).float(), x=(f(B, S, E) * rs.flip(0)[:, None]).float())


def sddmm_refs(inp, scale: float, clamp: float):
    scale = f32(scale)
    E, row_of = inp['E'], inp['row_of']
    B = inp['q'].size(0)
    bi = torch.arange(B)[:, None]
    prod = inp['q'].double()[:, row_of] * inp['k'].double()[bi, inp['indices'].long()]
    lpe = E // 16 if E in (64, 128) else 1 << max(0, (E // 4 - 1).bit_length())
    depth = (16 if E in (64, 128) else 4) + int(math.log2(lpe))
    raw = scale * prod.sum(-1)
    bound = scale * X.fp32_tree_bound(prod.abs().sum(-1), depth) + U * raw.abs()
    return {'out': (raw.clamp(-clamp, clamp) if clamp > 0 else raw, bound * SECOND)}


def spmm_refs(inp, transposed: bool):
    E, S, row_of = inp['E'], inp['S'], inp['row_of']
    B, nnz = inp['values'].shape
    bi = torch.arange(B)[:, None]
    cols = inp['indices'].long()
    rows = row_of.expand(B, nnz)
    src, dst = (rows, cols) if transposed else (cols, rows)
    terms = inp['values'].double()[..., None] * inp['x'].double()[bi, src]
    at = dst[..., None].expand(B, nnz, E)
    y = torch.zeros([B, S, E], dtype=torch.float64).scatter_add_(1, at, terms)
    mag = torch.zeros([B, S, E], dtype=torch.float64).scatter_add_(1, at, terms.abs())
    length = torch.zeros([B, S], dtype=torch.float64).scatter_add_(1, dst, torch.ones([B, nnz], dtype=torch.float64))
    rounds = ((length + 63) / 64).floor()
    if E in (64, 128):
        depth = 16 * rounds + 5 + (S // 512 if transposed and E == 64 and S > 512 and S % 512 == 0 else 0)
    else:
        lpe = 1 << max(0, (E // 4 - 1).bit_length())
        depth = lpe * rounds + int(math.log2(64 // lpe))
    return {'y': (y, X.fp32_tree_bound(mag, depth[..., None]))}


# ------------------------------------------------------------------------------ fused attention
#
# fused_attention.hip, E = 64, uniform rows of Z entries; per (sample, head) slice, in fp64 with the
# error every step can add, first order, from the magnitudes of its own operands:
#   s = clamp(scale q.k)     16 fmas per lane, 2 butterfly levels: tree_bound(sum |q k|, 18) scale, one
#                            rounding for the scale; the clamp is 1-Lipschitz
#   e = mask expf(s)         e (ds + EXPF_ULPS u)
#   R = max(1e-9, sum e)     4 additions per lane, the quad (2), the four entry groups (2): depth 8, + sum de
#   attn = fl(fl(1 / R) e)   attn (dR / R + (DIV_ULPS + 1) u) + de / R
#   y = sum attn v[col]      16 fmas per lane, the four entry groups: tree_bound(sum attn |v|, 18) + sum dattn |v|
# Backward, on the scores and attn it is GIVEN (the forward's stored ones):
#   dP = dy.v[col]           tree_bound(sum |dy v|, 18)
#   c = max(1e-9, sum mask attn dP)    the product, then depth 8: tree_bound(., 9) + sum attn ddP
#   dS = scale attn (dP - c) where |score| < clamp, else 0:  scale attn (ddP + dc + u |dP - c|) + 2 u |dS|
#   grad_q = sum dS k[col]   tree_bound(sum |dS k|, 18) + sum ddS |k|
# CAUSAL kernels stage K / V as the rows need them: the scores of masked entries are then unspecified
# (the kernel's header), so the causal cases use patterns without masked entries.

def attention_inputs(N: int, H: int, S: int, Z: int, causal: bool, seed: int):
    gen = torch.Generator().manual_seed(seed)
    B, E = N * H, 64
    q, k, v = [torch.randn([N, S, H, E], generator=gen) for _ in range(3)]
    q = q * 3.0                                                   # some scores beyond the clamp
    v = v * torch.pow(2.0, -row_exponents(E).float())              # columns: a row of y mixes many rows of v
    dy = torch.randn([B, S, E], generator=gen) * torch.pow(2.0, -row_exponents(S, 3).float()).view(1, S, 1)
    cols = torch.randint(0, S, [B, S, Z], generator=gen)
    if causal:                                                    # lookup's: columns <= row, column-0 padding
        rows = torch.arange(S).view(1, S, 1)
        cols = torch.where(torch.arange(Z).view(1, 1, Z) <= rows, cols % (rows + 1), torch.zeros_like(cols))
    return dict(q=q, k=k, v=v, dy=dy, indices=cols.view(B, S * Z).int(), S=S, Z=Z, scale=E ** -0.5, clamp=10.0)


def _slices(t):
    N, S, H, E = t.shape
    return t.transpose(1, 2).reshape(N * H, S, E).double()


def _entries(dense, cols):
    return dense.gather(2, cols)                                  # [B, S, Z] of a [B, S, S] array


def _spread(vals, cols, S):
    return torch.zeros([vals.size(0), S, S], dtype=torch.float64).scatter_add_(2, cols, vals)


def attention_forward_refs(inp, expf=EXPF_ULPS):
    S, Z, scale, clamp = inp['S'], inp['Z'], inp['scale'], inp['clamp']
    q, k, v = (_slices(inp[n]) for n in ('q', 'k', 'v'))
    B = q.size(0)
    cols = inp['indices'].long().view(B, S, Z)
    mask = (cols <= torch.arange(S).view(1, S, 1)).double()
    raw = scale * _entries(q @ k.transpose(1, 2), cols)
    ds = scale * X.fp32_tree_bound(_entries(q.abs() @ k.abs().transpose(1, 2), cols), 18) + U * raw.abs()
    s = raw.clamp(-clamp, clamp)
    e = mask * s.exp()
    de = e * (ds * (1 + 2 * ds) + expf * U)
    R = e.sum(-1, keepdim=True)
    dR = X.fp32_tree_bound(R, 8) + de.sum(-1, keepdim=True)
    den = R.clamp_min(FLOOR32)
    attn = e / den
    dattn = (attn * (dR / den + (DIV_ULPS + 1) * U) + de / den) * SECOND
    y = _spread(attn, cols, S) @ v
    dy_ = X.fp32_tree_bound(_spread(attn, cols, S) @ v.abs(), 18) + _spread(dattn, cols, S) @ v.abs()
    return {'scores': (s.view(B, -1), (ds * SECOND).view(B, -1)), 'attn': (attn.view(B, -1), dattn.view(B, -1)),
            'y': (y, dy_ * SECOND)}


def attention_backward_refs(inp, scores32, attn32):
    S, Z, scale, clamp = inp['S'], inp['Z'], inp['scale'], inp['clamp']
    k, v, dy = _slices(inp['k']), _slices(inp['v']), inp['dy'].double()
    B = k.size(0)
    cols = inp['indices'].long().view(B, S, Z)
    mask = (cols <= torch.arange(S).view(1, S, 1)).double()
    p = attn32.double().view(B, S, Z) * mask
    inside = (scores32.double().view(B, S, Z).abs() < clamp).double()
    dP = _entries(dy @ v.transpose(1, 2), cols)
    ddP = X.fp32_tree_bound(_entries(dy.abs() @ v.abs().transpose(1, 2), cols), 18)
    c = (p * dP).sum(-1, keepdim=True)
    dc = X.fp32_tree_bound((p * dP).abs().sum(-1, keepdim=True), 9) + (p * ddP).sum(-1, keepdim=True)
    c = c.clamp_min(FLOOR32)
    dS = scale * p * (dP - c) * inside
    ddS = (scale * p * (ddP + dc + U * (dP - c).abs()) * inside + 2 * U * dS.abs()) * SECOND
    gq = _spread(dS, cols, S) @ k
    dgq = X.fp32_tree_bound(_spread(dS.abs(), cols, S) @ k.abs(), 18) + _spread(ddS, cols, S) @ k.abs()
    N, _, H, E = inp['k'].shape
    back = lambda t: t.view(N, H, S, E).transpose(1, 2)                          # -> [N, S, H, E]
    return {'grad_raw': (dS.view(B, -1), ddS.view(B, -1)), 'grad_q': (back(gq), back(dgq * SECOND))}


# ------------------------------------------------------------------------------------------- PQ
#
# pq_loss.hip, per D-dim sub-vector z of subspace m, W = table[m] [16, D]:
#   d_c = sum_i |z_i - W_ci|              D serial additions of rounded terms: relative gamma_(D + 1) =: rd
#   best = argmin_c d_c;  zq = W[best]
#   soft~_c = max(d_best, 1e-5) rcp(max(d_c, 1e-5))    relative 2 rd + (RCP_ULPS + 1) u (max is 1-Lipschitz)
#   soft_c = soft~_c rcp(sum soft~)       the sum: 16 additions (gamma_16); rcp and the product: RCP_ULPS + 1;
#                                         in all a RELATIVE error rs of every soft_c
#   zw_i = sum_c soft_c W_ci              at most 17 roundings: (gamma_17 + rs) sum_c soft_c |W_ci|
#   loss = sum (zw - zq)^2 + (z - zq)^2 / count     each difference rounds once; the squares go through one
#          lane's 2 D fmas per sub-vector it walks, 6 + 4 levels to the workgroup, ceil(nblk / 64) + 6 of the
#          finishing wave, and the product with 1 / count (2)
# Backward (g2 = 2 grad_loss / count: 3 roundings):
#   gzw = g2 (zw - zq), e2 = g2 (z - zq), hard = -gzw - e2
#   gs_c = <gzw, W_c>                     D / 2 fmas per half, one addition: gamma_(D/2 + 1)
#   dot = sum_c soft_c gs_c               8 fmas per lane, the pair of lanes: gamma_10
#   ga_c = soft_c (gs_c - dot);  gd_c = -ga_c rcp(max(d_c, 1e-5)) where d_c >= 1e-5, else 0
#   grad_z_i = e2_i - sum_c s_ci gd_c,  s_ci = +1 where W_ci >= z_i, else -1 (exact)         gamma_10
#   grad_weight[m, c, i] = sum over sub-vectors of soft_c gzw_i + [c == best] hard_i + s_ci gd_c: three fmas
#          per sub-vector a lane walks, the lanes of a wave that share (m, part), the 4 waves, then
#          pq_loss_table_reduce_kernel: ceil(nblk / 64) + 2 + 16
# Discontinuities (argmin, the 1e-5 floor): the builder resamples every sub-vector whose two smallest
# distances are closer than 64 rd of the larger, or that has a distance in (0, 1e-4); the placed ones (z
# equal to a codeword) sit exactly at distance 0.  Nothing is left out.
RCP_ULPS = 1          # __builtin_amdgcn_rcpf (v_rcp_f32): "1 ulp" in pq_loss.hip; no output isolates it, and every PQ
                      # output is within its bound with it (worst ratio 0.99, an accumulated grad_z)
PQ_FLOOR = float(torch.tensor(1e-5, dtype=torch.float32))


def _gamma(h):
    return h * U / (1 - h * U)


def pq_inputs(M: int, seed: int, parts: int = 1, N: int = 2, S: int = 256, H: int = 4, D: int = 8):
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn([M, 16, D], generator=gen)
    scale = torch.pow(2.0, -row_exponents(parts * N * S * H).float()).view(parts, N, S, H, 1)
    z = torch.randn([parts, N, S, H, M * D], generator=gen) * scale
    sub = z.view(-1, D)
    m_of = torch.arange(sub.size(0)) % M
    placed = torch.arange(0, sub.size(0), 50)
    sub[placed] = table[m_of[placed], torch.randint(0, 16, [placed.numel()], generator=gen)]

    def offenders():
        d = (sub.double()[:, None, :] - table.double()[m_of]).abs().sum(-1)
        two = d.sort(-1).values[:, :2]
        return ((two[:, 1] - two[:, 0] <= 64 * _gamma(D + 1) * two[:, 1]) | ((d > 0) & (d < 1e-4)).any(-1)).nonzero()[:, 0]
    for _ in range(10):
        bad = offenders()
        if bad.numel() == 0:
            break
        sub[bad] = torch.randn([bad.numel(), D], generator=gen)
    assert offenders().numel() == 0                                   # before the GPU is touched
    return dict(z=z, table=table, grad_loss=torch.tensor(0.75), parts=parts,
                prior=torch.randn(z.shape, generator=gen) * scale)


def pq_blocks(total: int, M: int, per_block: int = 256, cap: int = 512) -> int:
    """pq_loss_blocks of pq_loss.hip."""
    nblk = (total + 255) // 256
    if nblk > cap:
        unit = M // math.gcd(M, per_block)
        nblk = cap - cap % unit
    return nblk


def pq_refs(inp, accumulate: bool = False, rcp=None):
    rcp = RCP_ULPS if rcp is None else rcp
    z32, table, parts = inp['z'], inp['table'].double(), inp['parts']
    M, C, D = table.shape
    sub = z32.double().view(-1, D)
    total = sub.size(0)
    count = total // parts * D                                        # a mean per part
    W = table[torch.arange(total) % M]                                # [total, 16, D]
    d = (sub[:, None, :] - W).abs().sum(-1)
    best = d.argmin(-1)
    dc = d.clamp_min(PQ_FLOOR)
    softu = dc.gather(1, best[:, None]) / dc
    soft = softu / softu.sum(-1, keepdim=True)
    zq = W[torch.arange(total), best]
    zw = (soft[..., None] * W).sum(1)
    e1, e2 = zw - zq, sub - zq
    rd = _gamma(D + 1)
    rs = 2 * (2 * rd + (rcp + 1) * U) + _gamma(16) + (rcp + 1) * U
    dzw = (_gamma(17) + rs) * (soft[..., None] * W.abs()).sum(1)
    de1, de2 = dzw + U * e1.abs(), U * e2.abs()
    # loss
    nblk = pq_blocks(total, M)
    walked = (total + nblk * 256 - 1) // (nblk * 256)
    depth = 2 * D * walked + 1 + 6 + 4 + (nblk + 63) // 64 + 6 + 2
    T = (e1 ** 2 + e2 ** 2).sum()
    loss = T / count
    dloss = ((2 * e1.abs() * de1 + 2 * e2.abs() * de2).sum() + _gamma(depth) * T) / count
    refs = {'loss': (loss, dloss * SECOND)}
    # backward
    g2 = 2 * float(inp['grad_loss']) / count
    gzw, e2g = g2 * e1, g2 * e2
    dgzw = abs(g2) * de1 + 4 * U * gzw.abs()
    de2g = 5 * U * e2g.abs()
    hard = -gzw - e2g
    dhard = dgzw + de2g + U * hard.abs()
    gs = (gzw[:, None, :] * W).sum(-1)
    dgs = _gamma(D // 2 + 1) * (gzw[:, None, :] * W).abs().sum(-1) + (dgzw[:, None, :] * W.abs()).sum(-1)
    dot = (soft * gs).sum(-1, keepdim=True)
    ddot = _gamma(10) * (soft * gs).abs().sum(-1, keepdim=True) + (rs * soft * gs.abs() + soft * dgs).sum(-1, keepdim=True)
    ga = soft * (gs - dot)
    dga = (rs + U) * ga.abs() + soft * (dgs + ddot + U * (gs - dot).abs())
    live = (d >= PQ_FLOOR).double()
    gd = -ga / dc * live
    dgd = (dga / dc + gd.abs() * (rd + (rcp + 1) * U)) * live
    s = torch.where(W >= sub[:, None, :], 1.0, -1.0).double()
    gz = e2g - (s * gd[..., None]).sum(1)
    dgz = _gamma(10) * (e2g.abs() + gd.abs().sum(1, keepdim=True)) + de2g + dgd.sum(1, keepdim=True)
    if accumulate:
        gz = gz + inp['prior'].double().view(-1, D)
        dgz = dgz + U * gz.abs()
    refs['grad_z'] = (gz.view(z32.shape), (dgz * SECOND).view(z32.shape))
    onehot = torch.zeros_like(soft).scatter_(1, best[:, None], 1.0)
    terms = [soft[..., None] * gzw[:, None, :], onehot[..., None] * hard[:, None, :], s * gd[..., None]]
    dterm = rs * terms[0].abs() + soft[..., None] * dgzw[:, None, :] + onehot[..., None] * dhard[:, None, :] + dgd[..., None]
    nblk = pq_blocks(2 * total, M, 128)
    walked = (total + nblk * 128 - 1) // (nblk * 128)
    merge = int(math.log2(64 // (2 * M))) if M & (M - 1) == 0 else (64 + 2 * M - 1) // (2 * M) - 1
    depth = 3 * walked + merge + 4 + (nblk + 63) // 64 + 2 + 16
    by_m = lambda t: t.view(total // M, M, C, D).sum(0)
    gw = by_m(sum(terms))
    dgw = _gamma(depth) * by_m(sum(t.abs() for t in terms)) + by_m(dterm)
    refs['grad_weight'] = (gw, dgw * SECOND)
    return refs


# cdist.hip backward: grad_query[m, q, i] = sum_c s go[m, q, c], s = +1 where q_i > t_ci, else -1: a lane's 4
# codewords, the 4 lanes of a row (2 levels): depth 6.  grad_table[m, c, i] = -sum_q s go[m, q, c]: a lane
# walks rows_per_block / 64 rows, the 64 lanes that hold a codeword add into LDS one after another (64, in
# any order), then one addition per block.

def cdist_backward_refs(query32, table32, go32):
    q, t, go = query32.double(), table32.double(), go32.double()
    M, NQ, D = q.shape
    s = torch.where(q[:, :, None, :] > t[:, None, :, :], 1.0, -1.0).double()          # [M, NQ, C, D]
    gq = (s * go[..., None]).sum(2)
    mag = go.abs().sum(2, keepdim=True).expand(M, NQ, D)
    nblk = min(max((NQ + 2047) // 2048, 1), 256)
    rpb = (((NQ + nblk - 1) // nblk) + 63) // 64 * 64
    depth = rpb // 64 + 64 + nblk
    gt = -(s * go[..., None]).sum(1)
    return {'grad_query': (gq, X.fp32_tree_bound(mag, 6)),
            'grad_table': (gt, X.fp32_tree_bound(go.abs().sum(1)[..., None].expand_as(gt), depth))}
