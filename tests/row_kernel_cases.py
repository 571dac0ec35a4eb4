"""Inputs, float64 references and bounds of the row-kernel tests (test_gpu_row_kernels.py on the GPU, test_row_kernels_cpu.py
on the host): the towers' forward LayerNorm in its three output forms (mpreid_layernorm_f32), the head of every tower
(mpreid_tower_head_f32) and QuickGELU's backward (mpreid_quickgelu_backward_f32).  No GPU is needed here.

Every check is a function that returns `error / allowed` (its largest value over what it looks at): the GPU test asserts that
the kernel's output stays <= 1, the host test that every mutant a kernel could be lands >= MUTANT_FACTOR.  The bounds come from
the fp32 arithmetic itself, never from a kernel: for LayerNorm and the head, FACTOR times the figure that the fp32 host
restatement (torch.nn.functional.layer_norm in fp32, what model/clip/model.py:150-156 runs; @ proj in fp32; necks as one fused
multiply-add) reaches on the SAME rows against float64, and not below FLOOR.  The figure is the per-row relative L2 error, the
largest over the rows.  x - mean cancels on rows whose mean is large against their spread (`offset`, `tiny`): that is the
conditioning of the operation in fp32, not a defect, and it is why the bound is not one constant.  FACTOR = 4 covers the
kernels' summation order (a butterfly over 64 lanes) against the host's pairwise one."""
import functools

import torch
import torch.nn.functional as F

from text_cases import _ln64, rel_l2   # noqa: F401  (rel_l2: for the tests that import this module)

FACTOR, FLOOR = 4.0, 1e-6    # FLOOR: 16 fp32 ulp of a row's norm
BAR = 2e-5                   # the project's split-mode bar, met outright by the well-scaled groups
MUTANT_FACTOR = 100.0


def massive_rows(rows, width, seed):
    """(x, gamma) of a trained CLIP tower's residual stream: N(0, 1) rows with channel 5 at +1900 and channel W / 2 + 3 at -1900
    (in every third row only channel 5 is massive, at 2100), four gammas x30-100 and the massive channels' gamma 0.02"""
    g = torch.Generator().manual_seed(seed)
    c0, c1 = 5, width // 2 + 3
    x = torch.randn(rows, width, generator=g)
    x[:, c0] += 1900.0
    x[:, c1] -= 1900.0
    x[::3, c0] += 200.0
    x[::3, c1] += 1900.0
    gamma = 1.0 + 0.05 * torch.randn(width, generator=g)
    big = [c for c in torch.randperm(width, generator=g).tolist() if c not in (c0, c1)][:4]
    gamma[big] *= 30.0 + 70.0 * torch.rand(4, generator=g)
    gamma[[c0, c1]] = 0.02
    return x, gamma


def row_rel(got, want):
    """per-row relative L2 error in float64 -> [rows]; a row that is not finite counts as infinitely far"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    e = (got - want).norm(dim=-1) / want.norm(dim=-1)
    return torch.where(torch.isfinite(got).all(dim=-1), e, torch.full_like(e, float("inf")))


def figure(got, want):
    return float(row_rel(got, want).max())


def fma32(v, scale, shift):
    """fp32 fmaf(v, scale, shift): the product of two fp32 values is exact in float64, so one rounding counts"""
    return (v.double() * scale.double() + shift.double()).float()


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
#: 1, 2, 3, 3 and 4 of the kernel's register slots (256 columns each); 384 and 640 leave the last one half full
LN_WIDTHS = [128, 384, 640, 768, 1024]
#: below, at and above the four rows of a workgroup, and a ragged last workgroup behind several full ones
LN_ROWS = [1, 4, 5, 37]
LN_GROUPS = ("unit", "large", "massive", "offset", "tiny", "const")
LN_BAR_GROUPS = ("unit", "large", "massive")   # these meet BAR outright
CONST_VALUE = 3.25


@functools.lru_cache(maxsize=None)
def ln_inputs(width):
    """group -> (x [37, width], gamma, beta), fp32; beta is non-zero everywhere"""
    g = torch.Generator().manual_seed(7000 + width)
    rows = max(LN_ROWS)
    gamma = 1.0 + 0.05 * torch.randn(width, generator=g)
    beta = 0.3 * torch.randn(width, generator=g)
    beta = torch.where(beta.abs() < 0.01, torch.full_like(beta, 0.25), beta)
    xm, gm = massive_rows(rows, width, 2000 + width)
    x = {"unit": torch.randn(rows, width, generator=g), "large": 100.0 + 1e3 * torch.randn(rows, width, generator=g), "massive": xm,
         "offset": 1000.0 + torch.randn(rows, width, generator=g), "tiny": 0.5 + 1e-4 * torch.randn(rows, width, generator=g),
         "const": torch.full((rows, width), CONST_VALUE)}
    return {k: (v, gm if k == "massive" else gamma, beta) for k, v in x.items()}


def ln_host32(x, gamma, beta):
    return F.layer_norm(x.float(), (x.shape[-1],), gamma.float(), beta.float(), 1e-5)


class LnCase:
    """the first `rows` rows of a group at a width: inputs, the float64 output, the host's fp32 figure and the bounds from it.
    The figure is the GROUP's, taken over all its 37 rows, for every row count: the rows of a group are alike, the error of one
    row is one draw of the cancellation in x - mean, and the largest of 37 draws says what fp32 does to such rows where a
    single draw does not (a call on the first row alone is held to what the group is held to)"""

    def __init__(self, width, group, rows):
        x, self.gamma, self.beta = ln_inputs(width)[group]
        self.width, self.group, self.rows = width, group, rows
        self.x = x[:rows].contiguous()
        y64 = _ln64(x.double(), self.gamma.double(), self.beta.double())
        self.y64 = y64[:rows]
        self.host_figure = figure(ln_host32(x, self.gamma, self.beta), y64)
        self.bound = max(FACTOR * self.host_figure, FLOOR)              # on the per-row relative L2 of the fp32 form
        self.row_abs = self.bound * self.y64.norm(dim=1, keepdim=True)  # what that allows any one element of a row, [rows, 1]

    # form 0: got fp32 [rows, W] -> (the figure, figure / bound)
    def form0(self, got):
        fig = figure(got, self.y64)
        return fig, fig / self.bound

    # form 1: got fp16 [rows, W]; |y16 - y64| <= 2^-11 |y64| + 2^-25 (one rounding to fp16, half a subnormal step) + row_abs
    def form1(self, got):
        err = (got.detach().cpu().double() - self.y64).abs()
        return _worst(err, 2.0 ** -11 * self.y64.abs() + 2.0 ** -25 + self.row_abs)

    # form 2: got fp16 [rows, 2W] = [hi | lo] -> (the pair's error / allowed, |lo| / half an fp16 ulp of hi)
    def form2(self, got):
        W = self.width
        pair = got.detach().cpu().double()
        hi, lo = pair[:, :W], pair[:, W:]
        total = _worst((hi + lo - self.y64).abs(), self.row_abs + 2.0 ** -22 * self.y64.abs() + 2.0 ** -25)
        return total, _worst(lo.abs(), 0.5 * ulp16(hi))


def ulp16(h):
    """the fp16 ulp of every element of h (float64 holding fp16 values): 2^(e - 10) for 2^e <= |h| < 2^(e + 1), 2^-24 below 2^-14"""
    e = torch.floor(torch.log2(h.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10.0)


def _worst(err, allowed):
    r = err / allowed
    return float(torch.where(torch.isfinite(err), r, torch.full_like(r, float("inf"))).max())


@functools.lru_cache(maxsize=None)
def ln_case(width, group, rows=max(LN_ROWS)):
    return LnCase(width, group, rows)


def split_pair_host(y32):
    """hi = fp16(y), lo = fp16(y - hi) of fp32 values -> fp16 [rows, 2W] (the split precision's pair, on the host)"""
    hi = y32.half()
    return torch.cat([hi, (y32 - hi.float()).half()], dim=1)


# ---- what a LayerNorm kernel could be instead (float64, so that only the mistake separates them from the reference) ------
def ln_mutant_slot(case):
    """the last register slot's lane-to-column map reversed: lane l of the slot's n lanes writes the float4 of lane n - 1 - l"""
    W = case.width
    first = (W - 1) // 256 * 256
    y = case.y64.clone()
    y[:, first:] = case.y64[:, first:].reshape(case.rows, -1, 4).flip(1).reshape(case.rows, -1)
    return y


def ln_mutant_slots_swapped(case):
    """register slots 0 and 1 (columns 0 .. 255 and 256 .. 511) written to each other's columns; widths >= 512"""
    y = case.y64.clone()
    y[:, :256], y[:, 256:512] = case.y64[:, 256:512], case.y64[:, :256]
    return y


def ln_mutant_no_eps(case):
    x = case.x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var) * case.gamma.double() + case.beta.double()


def ln_mutant_swapped_halves(case):
    p = split_pair_host(case.y64.float())
    return torch.cat([p[:, case.width:], p[:, :case.width]], dim=1)


def ln_mutant_pair_shifted(case):
    """the lo half written one float4 (four columns) late"""
    p = split_pair_host(case.y64.float())
    return torch.cat([p[:, :case.width], torch.roll(p[:, case.width:], 4, dims=1)], dim=1)


# ----------------------------------------------------------------------------------------------------------------------
# the tower head
# ----------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(128, 64), (768, 512), (1024, 257), (256, 1)]   # (width, out_dim): out_dim below, across and off the 256 columns of a workgroup
HEAD_BATCHES = [1, 2, 3, 5, 9]                                 # odd and even against the two items of a workgroup, and > the four of head_ln
HEAD_TOKENS = 77
HEAD_CLS_TOKENS = 3                                            # the CLS form's items: 3 rows, or the row alone (item_stride = W)
#: the read-out rows of the row_of form by batch: 0, L - 1, and entries outside the prompt (-3, L + 5, -1, L) that must be clamped
_L = HEAD_TOKENS
HEAD_ROW_OF = {1: [_L + 5], 2: [-3, _L + 5], 3: [_L - 1, -3, _L + 5], 5: [0, _L - 1, -3, _L + 5, 40],
               9: [0, _L - 1, -3, _L + 5, 40, 1, _L - 2, -1, _L]}
HEAD_NECKS = ("none", "both", "bn", "bnp")


def clamp_rows(row_of, tokens):
    return [min(max(int(e), 0), tokens - 1) for e in row_of]


@functools.lru_cache(maxsize=None)
def head_weights(width, out_dim):
    """ln gamma (the massive rows' own: x30-100 and 0.02 entries) and beta != 0, proj ~ N(0, 1 / width) as CLIP initialises it,
    and the two eval-BatchNorm necks as (scale, shift)"""
    g = torch.Generator().manual_seed(9000 + 7 * width + out_dim)
    _, gamma = massive_rows(1, width, 3000 + width)
    beta = 0.3 * torch.randn(width, generator=g)
    proj = torch.randn(width, out_dim, generator=g) * width ** -0.5
    bn = (0.5 + torch.rand(width, generator=g), 0.2 * torch.randn(width, generator=g))
    bnp = (0.5 + torch.rand(out_dim, generator=g), 0.2 * torch.randn(out_dim, generator=g))
    return gamma, beta, proj, bn, bnp


@functools.lru_cache(maxsize=None)
def head_items(width, tokens, batch=max(HEAD_BATCHES)):
    """x [batch, tokens, width]: even items N(0, 1) rows, odd items the massive rows"""
    g = torch.Generator().manual_seed(11000 + 13 * width + tokens)
    x = torch.randn(batch, tokens, width, generator=g)
    for b in range(1, batch, 2):
        x[b] = massive_rows(tokens, width, 4000 + width + b)[0]
    return x


class HeadRef:
    """the float64 head of the rows `rows` [B, W] (already picked and clamped), the host's fp32 restatement of it, and per
    output piece the bound: FACTOR x the host's figure, not below FLOOR"""

    def __init__(self, rows, width, out_dim):
        self.gamma, self.beta, self.proj, self.bn, self.bnp = head_weights(width, out_dim)
        self.width, self.out_dim = width, out_dim
        self.y64 = _ln64(rows.double(), self.gamma.double(), self.beta.double())
        self.p64 = self.y64 @ self.proj.double()
        self.y32 = ln_host32(rows, self.gamma, self.beta)
        self.p32 = self.y32 @ self.proj

    def want(self, necks, mutant=None):
        """(ln half, proj half) in float64 and their fp32 host restatement under a neck setting of HEAD_NECKS.
        mutant 'wrong_half': the bn neck gates the proj half and the bnp neck the ln half (each neck's own vectors, indexed
        modulo their length)"""
        on_ln, on_p = necks in ("both", "bn"), necks in ("both", "bnp")
        if mutant == "wrong_half":
            on_ln, on_p = on_p, on_ln
        ln64, p64, ln32, p32 = self.y64, self.p64, self.y32, self.p32
        if on_ln:
            s, b = self.bn if mutant is None else (_tile(t, self.width) for t in self.bnp)
            ln64, ln32 = ln64 * s.double() + b.double(), fma32(ln32, s, b)
        if on_p:
            s, b = self.bnp if mutant is None else (_tile(t, self.out_dim) for t in self.bn)
            p64, p32 = p64 * s.double() + b.double(), fma32(p32, s, b)
        return (ln64, p64), (ln32, p32)

    def bounds(self, necks):
        """piece -> (float64 value, bound) for 'y', 'ln' (out[:, :W]) and 'proj' (out[:, out_col:])"""
        (ln64, p64), (ln32, p32) = self.want(necks)
        pieces = {"y": (self.y64, self.y32), "ln": (ln64, ln32), "proj": (p64, p32)}
        return {k: (w64, max(FACTOR * figure(w32, w64), FLOOR)) for k, (w64, w32) in pieces.items()}


def _tile(t, n):
    return t[torch.arange(n) % t.shape[0]]


@functools.lru_cache(maxsize=None)
def head_ref(width, out_dim, form, batch):
    """form 'cls': row 0 of items 0 .. batch - 1 (the same rows whether the items are 3 rows or 1 row long); 'row_of': the
    clamped rows of HEAD_ROW_OF[batch] in items of HEAD_TOKENS rows"""
    if form == "cls":
        rows = head_items(width, HEAD_CLS_TOKENS)[:batch, 0]
    else:
        x = head_items(width, HEAD_TOKENS)
        rows = torch.stack([x[b, e] for b, e in enumerate(clamp_rows(HEAD_ROW_OF[batch], HEAD_TOKENS))])
    return HeadRef(rows.contiguous(), width, out_dim)


#: off-by-one clamps a kernel could have instead of [0, L - 1]: name -> row index used for entry e
WRONG_CLAMPS = {
    "upper_at_L": lambda e, L: min(max(e, 0), L),             # e > L - 1 tested as e > L
    "upper_at_L_minus_2": lambda e, L: min(max(e, 0), L - 2),
    "lower_at_1": lambda e, L: min(max(e, 1), L - 1),
}


# ----------------------------------------------------------------------------------------------------------------------
# QuickGELU backward
# ----------------------------------------------------------------------------------------------------------------------
GELU_SIZES = [4, 1020, 1024, 1028, 4 * 65537]   # one float4; around the 256 threads of a workgroup; more than 65 536 float4
GELU_ULPS = 8.0                                  # one expf, one division, three roundings
GELU_ABS = 1e-30                                 # x |d|: below it the sigmoid is a subnormal fp32 number or flushed to zero


@functools.lru_cache(maxsize=None)
def gelu_case(n):
    """(u, d, float64 d * (s + 1.702 u s (1 - s))): u uniform in -30 .. 30 with exact 0 and +-88 (expf saturates) placed in it,
    d ~ N(0, 1) with exact zeros"""
    g = torch.Generator().manual_seed(13000 + n)
    u = torch.rand(n, generator=g) * 60.0 - 30.0
    d = torch.randn(n, generator=g)
    special = torch.tensor([0.0, 88.0, -88.0, -0.0 if n > 8 else -1.5])   # (n = 4: one ordinary value among the special ones)
    u[:4] = special[torch.randperm(4, generator=g)]
    if n > 8:
        u[n - 3:] = torch.tensor([88.0, 0.0, -88.0])
        d[5::7] = 0.0
    return u, d, gelu_f64(u, d)


def gelu_f64(u, d, second=1.0):
    """second: the factor on the slope's second term (1: the reference; 0 and -1: the mutants)"""
    u64, d64 = u.double(), d.double()
    s = torch.sigmoid(1.702 * u64)
    return d64 * (s + second * 1.702 * u64 * s * (1.0 - s))


def gelu_host32(u, d):
    """the kernel's expressions in fp32 on the host"""
    sg = 1.0 / (1.0 + torch.exp(-1.702 * u.float()))
    return d.float() * fma32(1.702 * u.float() * sg, 1.0 - sg, sg)


def gelu_ulps(got, want, d):
    """elementwise |got - want| in units of 2^-24 |want| + GELU_ABS |d| / GELU_ULPS: the largest"""
    got, want = got.detach().cpu().double(), want.double()
    return _worst((got - want).abs(), 2.0 ** -24 * want.abs() + GELU_ABS * d.double().abs() / GELU_ULPS + 1e-300)


def gelu_cond(got, u, d):
    """elementwise |got - want| against 8 max(1, |1.702 u|) 2^-24 |d| (s + |t|) + GELU_ABS |d|, t = 1.702 u s (1 - s): the largest
    ratio.  The slope s + t crosses zero near u = -0.75, where s and t cancel and no bound relative to the result can hold, so
    this one is relative to |s| + |t|; and each of the eight roundings on the way (the constant, the product in expf's argument,
    expf, the sum, the division, 1 - s, the product t, the final sum) is amplified by at most a = |1.702 u|: the argument's
    rounding by expf, the error of s by the factor a in t."""
    u64, d64 = u.double(), d.double()
    s = torch.sigmoid(1.702 * u64)
    t = 1.702 * u64 * s * (1.0 - s)
    a = (1.702 * u64).abs().clamp_min(1.0)
    allowed = GELU_ULPS * a * 2.0 ** -24 * d64.abs() * (s + t.abs()) + GELU_ABS * d64.abs() + 1e-300
    return _worst((got.detach().cpu().double() - d64 * (s + t)).abs(), allowed)


def gelu_allowed_ulps(n):
    """GELU_ULPS, or twice what the fp32 host restatement needs on the same data if that is more"""
    u, d, want = gelu_case(n)
    host = gelu_ulps(gelu_host32(u, d), want, d)
    return (GELU_ULPS if host <= GELU_ULPS else 2.0 * host), host


# ----------------------------------------------------------------------------------------------------------------------
# refusals: every call below must return its code before anything is launched
# ----------------------------------------------------------------------------------------------------------------------
def refusals(L, lib, p):
    """[(what, return code, expected code)] of the three entry points' refusals; p: a 16-byte aligned address (never
    dereferenced: every call fails its checks, or has nothing to do)"""
    A, U = lib.ERR_ARG, lib.ERR_UNSUPPORTED
    ln, head, gelu = L.mpreid_layernorm_f32, L.mpreid_tower_head_f32, L.mpreid_quickgelu_backward_f32
    out = []

    def add(what, rc, want):
        msg = L.mpreid_last_error().decode("utf-8", "replace")
        out.append((what, rc, want, msg))

    for i, name in ((0, "x"), (3, "gamma"), (4, "beta"), (6, "out")):
        args = [p, 4, 128, p, p, 0, p, None]
        args[i] = None
        add("layernorm: NULL " + name, ln(*args), A)
        args[i] = p + 8
        add("layernorm: misaligned " + name, ln(*args), A)
    for w in (0, 64, 192, 1152, -128):
        add("layernorm: width %d" % w, ln(p, 4, w, p, p, 0, p, None), U)
    for form in (-1, 3):
        add("layernorm: form %d" % form, ln(p, 4, 128, p, p, form, p, None), A)
    add("layernorm: rows -1", ln(p, -1, 128, p, p, 0, p, None), A)
    for form in (0, 1, 2):
        add("layernorm: rows 0, form %d" % form, ln(p, 0, 128, p, p, form, p, None), 0)

    def head_args():
        return dict(x=p, item_stride=128, row_of=None, tokens=1, batch=2, width=128, out_dim=64, ln_g=p, ln_b=p, proj=p, bn_s=None,
                    bn_b=None, bnp_s=None, bnp_b=None, y=p, out=p, out_stride=192, out_col=128, ln_to_out=1, stream=None)

    def run_head(**kw):
        a = head_args()
        a.update(kw)
        return head(*a.values())
    for name in ("x", "ln_g", "ln_b", "proj", "y", "out"):
        add("head: NULL " + name, run_head(**{name: None}), A)
    add("head: misaligned x", run_head(x=p + 8), A)
    for name in ("row_of", "ln_g", "proj", "y", "out"):
        add("head: misaligned " + name, run_head(**{name: p + 2}), A)
    for w in (0, 64, 192, 1152):
        add("head: width %d" % w, run_head(width=w, out_col=w, out_stride=w + 64), U)
    add("head: half a neck", run_head(bn_s=p), A)
    add("head: half a proj neck", run_head(bnp_b=p), A)
    add("head: out_stride too small", run_head(out_stride=191), A)
    add("head: out_col inside the ln half", run_head(out_col=64), A)
    add("head: tokens 0", run_head(tokens=0), A)
    add("head: batch -1", run_head(batch=-1), A)
    add("head: out_dim 0", run_head(out_dim=0), A)
    add("head: batch 0", run_head(batch=0), 0)
    add("gelu: NULL u", gelu(None, p, 8, None), A)
    add("gelu: NULL d", gelu(p, None, 8, None), A)
    add("gelu: misaligned u", gelu(p + 4, p, 8, None), A)
    add("gelu: misaligned d", gelu(p, p + 8, 8, None), A)
    for n in (1, 2, 3, 5, 1022, -4):
        add("gelu: n %d" % n, gelu(p, p, n, None), A)
    add("gelu: n 0", gelu(p, p, 0, None), 0)
    return out
