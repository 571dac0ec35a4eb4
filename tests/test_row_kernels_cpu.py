"""The premises of tests/test_gpu_row_kernels.py, on the host: the bounds that test holds the kernels to (row_kernel_cases.py)
are met by the fp32 host restatement of each operation, the well-scaled row groups are far tighter than the ill-conditioned
ones, and every mistake a kernel could make instead -- a register slot's columns swapped or reversed, hi and lo swapped or one
float4 off, a clamp off by one, a neck on the wrong half, rstd without eps, the QuickGELU slope without or with the wrong sign
of its second term -- lands at least MUTANT_FACTOR = 100 times outside the bound of a named assertion there.  The mutants are
computed in float64, so nothing but the mistake separates them from the reference.  The entry points' refusals need no
device either: they happen before anything is launched."""
import pytest
import torch

import row_kernel_cases as rk
from mpreid import _lib


# ---- 1. LayerNorm: the host's fp32 figure, the bounds, the groups -----------------------------------------------------------------
@pytest.mark.parametrize("width", rk.LN_WIDTHS)
def test_layernorm_host_figures_and_bounds(width):
    """the fp32 host LayerNorm is inside each group's bound (by the factor the bound gives it) and, on its own output, inside the
    elementwise bounds of forms 1 and 2; unit / large / massive leave room under the 2e-5 bar; unit and large are >= 100 x
    tighter than offset and tiny (massive lies between: its figure is the massive channels' cancellation against 1900)"""
    fig = {}
    for group in rk.LN_GROUPS:
        for rows in rk.LN_ROWS:
            c = rk.ln_case(width, group, rows)
            host = rk.ln_host32(c.x, c.gamma, c.beta)
            f, ratio = c.form0(host)
            assert f <= c.host_figure and ratio <= 1.0 / rk.FACTOR + 1e-12, (group, rows, f)
            assert c.form1(host.half()) <= 1.0, (group, rows)
            total, lo = c.form2(rk.split_pair_host(host))
            assert total <= 1.0 and lo <= 1.0, (group, rows, total, lo)
        fig[group] = rk.ln_case(width, group).host_figure
        print("layernorm W = %d, %s rows: fp32 on the host %.3e, bound %.3e" % (width, group, fig[group], rk.ln_case(width, group).bound))
    for group in rk.LN_BAR_GROUPS:
        assert rk.ln_case(width, group).bound <= rk.BAR / 2, (group, fig[group])
    assert fig["const"] == 0.0 and rk.ln_case(width, "const").bound == rk.FLOOR
    assert 100.0 * max(fig["unit"], fig["large"]) <= min(fig["offset"], fig["tiny"]), fig
    # const rows: the output is beta, exactly, in float64 too
    c = rk.ln_case(width, "const")
    assert torch.equal(c.y64, c.beta.double().expand_as(c.y64)) and bool((c.beta != 0).all())


@pytest.mark.parametrize("width", rk.LN_WIDTHS)
def test_layernorm_mutants_are_far_outside_the_bounds(width):
    for group in rk.LN_GROUPS:
        c = rk.ln_case(width, group)
        # form 0's bound: a slot's lane map reversed (every width: at 128 it is slot 0), two slots swapped
        mutants = {"slot_reversed": rk.ln_mutant_slot(c)}
        if width >= 512:
            mutants["slots_swapped"] = rk.ln_mutant_slots_swapped(c)
        for name, y in mutants.items():
            ratio = c.form0(y)[1]
            assert ratio >= rk.MUTANT_FACTOR, (group, name, ratio)
            assert c.form1(y.half()) >= rk.MUTANT_FACTOR, (group, name)              # and form 1's elementwise bound
            assert c.form2(rk.split_pair_host(y.float()))[0] >= rk.MUTANT_FACTOR, (group, name)   # and form 2's
        # form 2's two assertions: the halves swapped breaks "|lo| <= half an ulp of hi", the lo half one float4 off breaks the sum
        assert c.form2(rk.ln_mutant_swapped_halves(c))[1] >= rk.MUTANT_FACTOR, group
        if group != "const":   # (lo of a constant row's output moves with beta only; beta's own lo is checked by the other groups)
            assert max(c.form2(rk.ln_mutant_pair_shifted(c))) >= rk.MUTANT_FACTOR, group
    # rstd without eps: not finite on const rows (0 * inf), 30 x off on tiny rows (variance 1e-8 against eps 1e-5)
    for group in ("const", "tiny"):
        c = rk.ln_case(width, group)
        ratio = c.form0(rk.ln_mutant_no_eps(c))[1]
        assert ratio >= rk.MUTANT_FACTOR, (group, ratio)
    assert not bool(torch.isfinite(rk.ln_mutant_no_eps(rk.ln_case(width, "const"))).any())
    # a lost last workgroup: rows 36 (37 % 4 = 1) left as the destination's NaN fill
    c = rk.ln_case(width, "unit")
    y = c.y64.clone()
    y[36:] = float("nan")
    assert c.form0(y)[1] == float("inf")


# ---- 2. the tower head ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,out_dim", rk.HEAD_SHAPES)
def test_head_host_figures_and_mutants(width, out_dim):
    """the host's fp32 head is inside every piece's bound; a clamp off by one and a neck on the wrong half are >= 100 x outside"""
    L = rk.HEAD_TOKENS
    for batch in rk.HEAD_BATCHES:
        for form in ("cls", "row_of"):
            ref = rk.head_ref(width, out_dim, form, batch)
            for necks in rk.HEAD_NECKS:
                (_, _), (ln32, p32) = ref.want(necks)
                b = ref.bounds(necks)
                for piece, got in (("y", ref.y32), ("ln", ln32), ("proj", p32)):
                    want, bound = b[piece]
                    assert rk.figure(got, want) <= bound, (batch, form, necks, piece)
                if necks != "none":
                    (ln_m, p_m), _ = ref.want(necks, mutant="wrong_half")
                    worst = max(rk.figure(ln_m, b["ln"][0]) / b["ln"][1], rk.figure(p_m, b["proj"][0]) / b["proj"][1])
                    assert worst >= rk.MUTANT_FACTOR, (batch, form, necks, worst)
        # the clamp: every wrong clamp moves at least one entry of this batch's row_of to another row, whose head is far away
        ref = rk.head_ref(width, out_dim, "row_of", batch)
        x = rk.head_items(width, L)
        b = ref.bounds("none")
        hit = set()
        for name, fn in rk.WRONG_CLAMPS.items():
            picked = [fn(e, L) for e in rk.HEAD_ROW_OF[batch]]
            if picked == rk.clamp_rows(rk.HEAD_ROW_OF[batch], L):
                continue
            flat = x.reshape(-1, width)   # (row L of item b is row 0 of item b + 1: what a read one row too far returns)
            rows = torch.stack([flat[min(i * L + e, flat.shape[0] - 1)] for i, e in enumerate(picked)])
            wrong = rk.HeadRef(rows, width, out_dim)
            for piece, got in (("y", wrong.y64), ("proj", wrong.p64)):
                assert rk.figure(got, b[piece][0]) / b[piece][1] >= rk.MUTANT_FACTOR, (batch, name, piece)
            hit.add(name)
        if batch >= 5:
            assert hit == set(rk.WRONG_CLAMPS), (batch, hit)
    assert {0, L - 1, -3, L + 5} <= set(rk.HEAD_ROW_OF[5]) and {0, L - 1, -3, L + 5} <= set(rk.HEAD_ROW_OF[9])


# ---- 3. QuickGELU backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rk.GELU_SIZES)
def test_quickgelu_backward_host_figure_and_mutants(n):
    """the fp32 host restatement against float64 in fp32 ulp of the result (printed: it decides the GPU test's allowance); the
    slope without its second term, or with that term's sign wrong, is >= 100 x outside on >= 40 % of the elements"""
    u, d, want = rk.gelu_case(n)
    allowed, host = rk.gelu_allowed_ulps(n)
    print("quickgelu backward n = %d: fp32 on the host %.2f ulp, allowed on the GPU %.2f" % (n, host, allowed))
    assert allowed >= rk.GELU_ULPS and host <= allowed
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(rk.gelu_host32(u, d)).all())
    assert {0.0, 88.0, -88.0} <= set(u.tolist())
    for second in (0.0, -1.0):
        mutant = rk.gelu_f64(u, d, second)
        assert rk.gelu_ulps(mutant, want, d) >= rk.MUTANT_FACTOR * allowed, (n, second)
        if n > 8:   # not one lucky element: at least 40 % of the array is that far out
            far = (mutant - want).abs() >= rk.MUTANT_FACTOR * allowed * 2.0 ** -24 * want.abs() + rk.GELU_ABS * d.double().abs()
            assert float((far & (d != 0)).double().mean()) >= 0.4, (n, second)


def test_quickgelu_conditioned_bound_holds_on_the_host_and_breaks_on_the_mutants():
    """8 ulp OF THE RESULT cannot hold everywhere: the slope s + 1.702 u s (1 - s) crosses zero near u = -0.75, and at |u| = 30
    expf's argument 51 carries a rounding of 2^-19 = 32 x 2^-24 of its own.  row_kernel_cases.gelu_cond states the bound that
    fp32 arithmetic does meet (relative to |s| + |t|, roundings amplified by |1.702 u|): the host restatement is inside it on
    every case, around the zero crossing and at the ends; the mutants are >= 100 x outside on >= 40 % of the elements"""
    g = torch.Generator().manual_seed(5)
    d = torch.ones(4096)
    around_zero = -0.8 + 0.1 * torch.rand(4096, generator=g)
    ends = torch.cat([-30.0 + torch.rand(2048, generator=g), 29.0 + torch.rand(2048, generator=g)])
    for u in (around_zero, ends):
        assert rk.gelu_cond(rk.gelu_host32(u, d), u, d) <= 1.0
    assert rk.gelu_ulps(rk.gelu_host32(around_zero, d), rk.gelu_f64(around_zero, d), d) > rk.GELU_ULPS
    for n in rk.GELU_SIZES:
        u, d, want = rk.gelu_case(n)
        ratio = rk.gelu_cond(rk.gelu_host32(u, d), u, d)
        print("quickgelu backward n = %d: fp32 on the host at %.3f of the conditioned bound" % (n, ratio))
        assert ratio <= 1.0, n
        for second in (0.0, -1.0):
            assert rk.gelu_cond(rk.gelu_f64(u, d, second), u, d) >= rk.MUTANT_FACTOR, (n, second)


# ---- 4. the entry points ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve_and_refuse_before_any_launch():
    """no device here: every refusal happens before the first HIP call, with a message; rows, batch or n of 0 is MPREID_OK"""
    L = _lib.load()
    for name in ("mpreid_layernorm_f32", "mpreid_tower_head_f32", "mpreid_quickgelu_backward_f32"):
        assert name in _lib.PROTOTYPES and hasattr(L, name), name
    assert _lib.VERSION == 102
    seen = rk.refusals(L, _lib, 0x1000)
    assert len(seen) >= 50
    for what, rc, want, msg in seen:
        assert rc == want, (what, rc, want)
        assert want == 0 or msg, what
    assert any(w == _lib.ERR_UNSUPPORTED for _, _, w, _ in seen) and any(w == 0 for _, _, w, _ in seen)
