"""The row kernels every tower runs between its GEMMs and its attention, each alone against float64: the forward LayerNorm in its
three output forms (layernorm_kernel<0 | 1 | 2> through mpreid_layernorm_f32), the head of every tower (head_ln_kernel +
head_proj_kernel through mpreid_tower_head_f32) and QuickGELU's backward (mpreid_quickgelu_backward_f32).  The entry points go
through the launchers the towers call.  Inputs, references, bounds and what each bound is derived from: row_kernel_cases.py;
that the bounds hold for fp32 arithmetic and that a wrong kernel lands >= 100 x outside them: test_row_kernels_cpu.py."""
import pytest
import torch

import row_kernel_cases as rk
from mpreid import _lib, ops

pytestmark = pytest.mark.gpu

G = 4                   # guard rows in front of and behind an output
NAN32 = 0x7FC12345      # NaN patterns the guards and the destinations are filled with
NAN16 = 0x7E11


def _guarded(rows, cols, dtype):
    """(the whole buffer as integers, the view of its middle `rows` rows in `dtype`): all of it a NaN pattern"""
    if dtype == torch.float32:
        buf = torch.full((G + rows + G, cols), NAN32, dtype=torch.int32, device="cuda")
    else:
        buf = torch.full((G + rows + G, cols), NAN16, dtype=torch.int16, device="cuda")
    return buf, buf[G:G + rows].view(dtype)


def _guards_intact(buf, rows):
    fill = NAN32 if buf.dtype == torch.int32 else NAN16
    return bool((buf[:G] == fill).all()) and bool((buf[G + rows:] == fill).all())


def _same_bits(a, b):
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---- 1. LayerNorm, form 0 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", rk.LN_WIDTHS)
def test_layernorm_fp32_against_float64(width):
    """per group of rows, the largest per-row relative L2 against float64 <= 4 x the fp32 host LayerNorm's figure on the group's
    37 rows (not below 1e-6); unit / large / massive also <= 2e-5 outright; const rows give beta to 1e-6; calls on the first 1,
    4 and 5 rows are held to the group's bound and give the bits those rows have in the call on all 37; in place gives the
    bits of out of place; the destination starts as NaN between guard rows that stay untouched.
    Measured on an MI355X (37 rows; kernel / fp32 on the host), W = 128, 384, 640, 768, 1024: see DESIGN.md section 14"""
    for group in rk.LN_GROUPS:
        c = rk.ln_case(width, group)
        whole = ops.layernorm(c.x.cuda(), c.gamma.cuda(), c.beta.cuda(), 0).clone()
        for rows in rk.LN_ROWS:
            c = rk.ln_case(width, group, rows)
            x, gamma, beta = c.x.cuda(), c.gamma.cuda(), c.beta.cuda()
            buf, out = _guarded(rows, width, torch.float32)
            assert ops.layernorm(x, gamma, beta, 0, out=out) is out
            torch.cuda.synchronize()
            assert _guards_intact(buf, rows), (group, rows)
            assert bool(torch.isfinite(out).all()), (group, rows)
            fig, ratio = c.form0(out)
            if rows == max(rk.LN_ROWS):
                print("layernorm form 0, W = %d, %s rows: %.3e (fp32 on the host %.3e, bound %.3e)"
                      % (width, group, fig, c.host_figure, c.bound))
            assert ratio <= 1.0, (group, rows, fig, c.bound)
            if group in rk.LN_BAR_GROUPS:
                assert fig <= rk.BAR, (group, rows, fig)
            # in place, between guard rows of its own
            ibuf, xin = _guarded(rows, width, torch.float32)
            xin.copy_(x)
            assert ops.layernorm(xin, gamma, beta, 0, out=xin) is xin
            torch.cuda.synchronize()
            assert _guards_intact(ibuf, rows) and _same_bits(xin, out) and _same_bits(out, whole[:rows]), (group, rows)
            assert torch.equal(x.cpu(), c.x)   # the out-of-place call left its input alone


# ---- 2. LayerNorm, forms 1 and 2 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", rk.LN_WIDTHS)
def test_layernorm_fp16_and_pair_forms_against_float64(width):
    """form 1, elementwise: |y16 - y64| <= 2^-11 |y64| + 2^-25 + the row's form-0 allowance.  form 2: |hi + lo - y64| <= the
    row's form-0 allowance + 2^-22 |y64| + 2^-25; |lo| <= half an fp16 ulp of hi (hi is the rounding of the value, not its
    truncation; and the halves lie at columns [0, W) and [W, 2W): swapped, this is off by orders of magnitude); hi has the
    bits of form 1.  NaN-filled destinations between guard rows, every row count"""
    for group in rk.LN_GROUPS:
        for rows in rk.LN_ROWS:
            c = rk.ln_case(width, group, rows)
            x, gamma, beta = c.x.cuda(), c.gamma.cuda(), c.beta.cuda()
            buf1, y16 = _guarded(rows, width, torch.float16)
            buf2, pair = _guarded(rows, 2 * width, torch.float16)
            assert ops.layernorm(x, gamma, beta, 1, out=y16) is y16 and ops.layernorm(x, gamma, beta, 2, out=pair) is pair
            torch.cuda.synchronize()
            assert _guards_intact(buf1, rows) and _guards_intact(buf2, rows), (group, rows)
            assert bool(torch.isfinite(y16).all()) and bool(torch.isfinite(pair).all()), (group, rows)
            r1 = c.form1(y16)
            total, lo = c.form2(pair)
            if rows == max(rk.LN_ROWS):
                print("layernorm W = %d, %s rows: form 1 at %.3f of its bound, form 2 at %.3f, |lo| at %.3f of half an ulp of hi"
                      % (width, group, r1, total, lo))
            assert r1 <= 1.0, (group, rows, r1)
            assert total <= 1.0 and lo <= 1.0, (group, rows, total, lo)
            assert _same_bits(pair[:, :width], y16), (group, rows)


# ---- 3. the tower head ---------------------------------------------------------------------------------------------------------------
def _head_x(width, form, batch, cls_tokens):
    """(x on the device, item_stride, row_of, tokens) of a head call"""
    if form == "cls":
        x = rk.head_items(width, rk.HEAD_CLS_TOKENS)[:batch, :cls_tokens].contiguous()
        return x.cuda(), cls_tokens * width, None, 1
    x = rk.head_items(width, rk.HEAD_TOKENS)[:batch].contiguous()
    return x.cuda(), rk.HEAD_TOKENS * width, torch.tensor(rk.HEAD_ROW_OF[batch], dtype=torch.int32).cuda(), rk.HEAD_TOKENS


HEAD_FORMS = [("cls", rk.HEAD_CLS_TOKENS), ("cls", 1), ("row_of", rk.HEAD_TOKENS)]   # item_stride = L * W, = W, and the row_of form


@pytest.mark.parametrize("width,out_dim", rk.HEAD_SHAPES)
def test_tower_head_against_float64(width, out_dim):
    """y, out[:, :W] and out[:, out_col:] each against float64 (for row_of, of the CLAMPED rows), per-row relative L2, the
    largest over the items <= 4 x the fp32 host restatement's (layer_norm, @ proj, fused multiply-add necks), not below 1e-6.
    Every batch, both item strides of the CLS form, row_of entries 0, L - 1 and outside the prompt, the necks none / both /
    each alone, ln_to_out on (out_stride W + out_dim, out_col W: the image towers) and off (out_stride out_dim, out_col 0: the
    text tower and the training forward).  out lies between NaN guard rows; with ln_to_out off it is [B, W + out_dim] with the
    projection at column W, and columns [0, W) must keep their fill"""
    gamma, beta, proj, bn, bnp = rk.head_weights(width, out_dim)
    worst = {"y": 0.0, "ln": 0.0, "proj": 0.0}
    for batch in rk.HEAD_BATCHES:
        for form, cls_tokens in HEAD_FORMS:
            x, stride, row_of, tokens = _head_x(width, form, batch, cls_tokens)
            ref = rk.head_ref(width, out_dim, form, batch)
            for necks in rk.HEAD_NECKS:
                want = ref.bounds(necks)
                kw = dict(bn=bn if necks in ("both", "bn") else None, bnp=bnp if necks in ("both", "bnp") else None)
                # the image towers' concat
                buf, out = _guarded(batch, width + out_dim, torch.float32)
                y, o = ops.tower_head(x, stride, row_of, tokens, batch, gamma, beta, proj, ln_to_out=True, out=out, **kw)
                torch.cuda.synchronize()
                assert o is out and _guards_intact(buf, batch), (batch, form, necks)
                for piece, got in (("y", y), ("ln", out[:, :width]), ("proj", out[:, width:])):
                    w64, bound = want[piece]
                    fig = rk.figure(got, w64)
                    worst[piece] = max(worst[piece], fig / bound)
                    assert fig <= bound, (batch, form, cls_tokens, necks, piece, fig, bound)
                # the text tower's form: [B, out_dim] alone ...
                buf2, out2 = _guarded(batch, out_dim, torch.float32)
                y2, _ = ops.tower_head(x, stride, row_of, tokens, batch, gamma, beta, proj, ln_to_out=False, out=out2, **kw)
                # ... and at column W of a wider row, whose first W columns are not the head's to write
                buf3, out3 = _guarded(batch, width + out_dim, torch.float32)
                ops.tower_head(x, stride, row_of, tokens, batch, gamma, beta, proj, ln_to_out=False, out=out3, out_col=width, **kw)
                torch.cuda.synchronize()
                assert _guards_intact(buf2, batch) and _guards_intact(buf3, batch), (batch, form, necks)
                assert bool((out3[:, :width].view(torch.int32) == NAN32).all()), (batch, form, necks)
                assert _same_bits(out2, out[:, width:]) and _same_bits(out3[:, width:], out2) and _same_bits(y2, y), (batch, form, necks)
    print("tower head (%d, %d): worst figure / bound over the cases: y %.3f, ln half %.3f, proj half %.3f"
          % (width, out_dim, worst["y"], worst["ln"], worst["proj"]))


@pytest.mark.parametrize("width,out_dim", rk.HEAD_SHAPES)
def test_tower_head_item_bits_do_not_depend_on_the_batch(width, out_dim):
    """an item has the same bits at any position in any batch, odd ones included (two items share a workgroup of the projection,
    four one of the LayerNorm), whichever way it is addressed: CLS with either item stride, or row_of naming the same row"""
    gamma, beta, proj, bn, bnp = rk.head_weights(width, out_dim)
    L = rk.HEAD_TOKENS
    items = rk.head_items(width, L)          # [9, L, W]
    picks = rk.clamp_rows(rk.HEAD_ROW_OF[9], L)
    full = items.cuda()
    _, base = ops.tower_head(full, L * width, torch.tensor(rk.HEAD_ROW_OF[9], dtype=torch.int32).cuda(), L, 9, gamma, beta, proj,
                             bn=bn, bnp=bnp)
    base = base.clone()
    for order in ([4], [8, 0], [2, 7, 5], [6, 1, 3, 8, 2], [8, 7, 6, 5, 4, 3, 2, 1, 0]):
        rows = torch.stack([items[i, picks[i]] for i in order]).cuda()    # the read-out rows alone: the CLS form, item_stride = W
        _, out = ops.tower_head(rows, width, None, 1, len(order), gamma, beta, proj, bn=bn, bnp=bnp)
        for k, i in enumerate(order):
            assert _same_bits(out[k], base[i]), (order, k)
        sub = items[order].contiguous().cuda()
        ro = torch.tensor([picks[i] for i in order], dtype=torch.int32).cuda()
        _, out = ops.tower_head(sub, L * width, ro, L, len(order), gamma, beta, proj, bn=bn, bnp=bnp)
        for k, i in enumerate(order):
            assert _same_bits(out[k], base[i]), (order, k)


# ---- 4. QuickGELU backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rk.GELU_SIZES)
def test_quickgelu_backward_against_float64(n):
    """elementwise against d (s + 1.702 u s (1 - s)) in float64: within 8 fp32 ulp of the result (+ 1e-30 |d|) -- or, where the
    fp32 host restatement needs more than 8 on the same data, twice its figure (it does, 84 .. 6335 ulp for n >= 1020: the slope
    crosses zero near u = -0.75, and expf's argument carries a rounding of its own, 32 ulp at |u| = 30) -- AND within the bound
    that does not depend on such luck, row_kernel_cases.gelu_cond: 8 max(1, |1.702 u|) ulp of |s| + |t|.  Finite at +-88; a d
    of zero stays zero to the bit; u is not written; the floats behind n keep their bits"""
    u, d, want = rk.gelu_case(n)
    allowed, host = rk.gelu_allowed_ulps(n)
    tail = 8
    ubuf = torch.full((n + tail,), float("nan"), device="cuda")
    ubuf[:n] = u.cuda()
    dbuf = torch.full((n + tail,), NAN32, dtype=torch.int32, device="cuda")
    dv = dbuf[:n].view(torch.float32)
    dv.copy_(d.cuda())
    assert ops.quickgelu_backward(ubuf[:n], dv) is dv
    torch.cuda.synchronize()
    assert bool((dbuf[n:] == NAN32).all()) and bool(torch.isnan(ubuf[n:]).all()) and torch.equal(ubuf[:n].cpu(), u)
    got = dv.cpu()
    assert bool(torch.isfinite(got).all())
    special = (u.abs() == 88.0)
    assert int(special.sum()) >= 2 and bool(torch.isfinite(got[special]).all())
    assert bool((got[d == 0] == 0.0).all())
    ulps, cond = rk.gelu_ulps(got, want, d), rk.gelu_cond(got, u, d)
    print("quickgelu backward n = %d: %.2f ulp of the result (fp32 on the host %.2f, allowed %.2f); %.3f of the conditioned bound"
          % (n, ulps, host, allowed, cond))
    assert ulps <= allowed, (n, ulps, allowed)
    assert cond <= 1.0, (n, cond)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_call_intact():
    """every refusal of the three entry points returns its code with a message, launches nothing, and the next good call of each
    entry point is right"""
    L = _lib.load()
    c = rk.ln_case(128, "unit", 5)
    x, gamma, beta = c.x.cuda(), c.gamma.cuda(), c.beta.cuda()
    u, d, want = rk.gelu_case(1028)
    ref = rk.head_ref(128, 64, "cls", 3)
    hx, stride, _, _ = _head_x(128, "cls", 3, 1)
    hg, hb, hp, _, _ = rk.head_weights(128, 64)

    def good():
        assert c.form0(ops.layernorm(x, gamma, beta))[1] <= 1.0
        assert rk.gelu_cond(ops.quickgelu_backward(u.cuda(), d.cuda()), u, d) <= 1.0
        y, out = ops.tower_head(hx, stride, None, 1, 3, hg, hb, hp)
        b = ref.bounds("none")
        assert rk.figure(y, b["y"][0]) <= b["y"][1] and rk.figure(out[:, 128:], b["proj"][0]) <= b["proj"][1]

    good()
    scratch = torch.zeros(4096, dtype=torch.float32, device="cuda")   # a real, 16-byte aligned address for the pointer arguments
    seen = rk.refusals(L, _lib, scratch.data_ptr())
    torch.cuda.synchronize()
    for what, rc, want_rc, msg in seen:
        assert rc == want_rc, (what, rc, want_rc)
        assert want_rc == 0 or msg, what
    assert bool((scratch == 0).all())
    good()
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_UNSUPPORTED):
        ops.layernorm(torch.zeros((4, 192), device="cuda"), torch.ones(192), torch.zeros(192))
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_ARG):
        ops.quickgelu_backward(torch.zeros(6, device="cuda"), torch.zeros(6, device="cuda"))
    good()
