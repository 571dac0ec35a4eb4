"""Every attention kernel form called directly through its seam, every written row against float64.

csrc/attention.hip holds fifteen attention kernels behind three dispatchers (the table of test_gpu_attention_forms.py): six fp16 forms
and five split forms with K / V resident in LDS, the streaming kernel above 256 tokens in both operand types, and the two all-fp32
kernels (resident up to 320 tokens, 128-key chunks above).  test_gpu_attention_direct.py does this for one of them,
attention_split_kernel<8,4,XKEY> at L = 129; here are all of them, through ops.vit_attention (fp16 input: the fp16 mode, fp32
input: the split mode) and ops.vit_attention_f32, in one process and without MPREID_TUNE.

Token counts, shapes, batches, data kinds and q_tiles: attention_direct_cases (FORMS_TOKENS, F32_TOKENS, forms_shapes, kinds,
q_tiles_of); the premises of the data are asserted in float64 by test_attention_direct_premises.py, which needs no GPU.

Per call (attention_direct_cases.checked_call): `out` between guard rows and pre-filled with a NaN pattern; every written row
finite; every row that must not be written and every guard row still the pattern; for B > 1 image i equal to the B = 1 call on
its slab, bit for bit; a second identical call the same bits.  Across q_tiles: the rows written under q_tiles = n > 0 carry the
bits of the same rows under q_tiles = 0 ("a tile's arithmetic does not depend on g, tpg or the batch").  The error figure is
error_figure (slab-relative, over the written rows) against attention_f64 of the operands as the kernel gets them.

Bounds -- none fitted to the code under test: split 2e-5 (text_cases.BOUND_SPLIT, the project's bar for a split attention kernel
at its own seam), fp32 2e-5 (BOUND["fp32"] of test_gpu_attention_forms.py), fp16 4 * 2^-11 (derived at
attention_direct_cases.BOUND_F16).  Every case prints an ATTFORMS line with its figure beside host_fp32, the same figure of
torch's fp32 evaluation of the formula on the CPU; profiles/attention_direct_forms.log is the output of one run on an MI355X,
for information: the measured figures are NOT the bounds, which would pin the test to the code it tests."""
import ctypes as C
import functools

import pytest
import torch

import attention_direct_cases as adc

pytestmark = pytest.mark.gpu

DTYPE = {"fp16": torch.float16, "split": torch.float32, "fp32": torch.float32}
BOUND = {"fp16": adc.BOUND_F16, "split": adc.BOUND_SPLIT, "fp32": adc.BOUND_F32}


@functools.lru_cache(maxsize=2)
def reference(prec, tokens, width, heads, batch, kind):
    """-> (operands on the host, float64 attention, slab scales, torch's fp32 attention on the host)"""
    host = adc.make_qkv(width, heads, batch, kind, tokens, DTYPE[prec])
    return host, adc.attention_f64(host, batch, heads), adc.slab_scale(host, batch, heads), adc.attention_host_f32(host, batch, heads)


def run_case(prec, tokens, width, heads, batch, kind):
    """every q_tiles of one case: the checks of checked_call, the bit agreement across q_tiles and the bound; every figure is
    printed before anything about it is asserted"""
    host, want, scale, host32 = reference(prec, tokens, width, heads, batch, kind)
    qkv = host.cuda()
    f32 = prec == "fp32"
    full, bad = None, []
    for q_tiles in ([0] if f32 else adc.q_tiles_of(tokens, kind)):
        tag = (prec, tokens, (width, heads), batch, kind)
        got, bits = adc.checked_call(qkv, batch, tokens, heads, q_tiles, f32=f32, tag=tag)
        rows = adc.written_rows(tokens, q_tiles)
        err = adc.error_figure(got, want, scale, rows=rows)
        print("ATTFORMS prec=%s L=%d shape=(%d,%d) B=%d kind=%s q_tiles=%d err=%.3e host_fp32=%.3e"
              % (prec, tokens, width, heads, batch, kind, q_tiles, err, adc.error_figure(host32, want, scale, rows=rows)))
        if not err <= BOUND[prec]:
            bad.append((q_tiles, "error figure", err, BOUND[prec]))
        if q_tiles == 0:
            full = bits
        elif not torch.equal(bits[:, :rows], full[:, :rows]):
            differ = (bits[:, :rows] != full[:, :rows]).any(-1).nonzero()
            bad.append((q_tiles, "rows whose bits differ from the q_tiles = 0 call [image, row]", differ[:8].tolist()))
    assert not bad, (prec, tokens, (width, heads), batch, kind, bad)


def _cases(tokens_list, shapes):
    return [pytest.param(t, w, h, b, k, id="L%d-%dx%d-B%d-%s" % (t, w, h, b, k))
            for t in tokens_list for w, h, b in shapes(t) for k in adc.kinds(t)]


@pytest.mark.parametrize("tokens,width,heads,batch,kind", _cases(adc.FORMS_TOKENS, adc.forms_shapes))
@pytest.mark.parametrize("prec", ["fp16", "split"])
def test_attention_forms_vs_float64(prec, tokens, width, heads, batch, kind):
    run_case(prec, tokens, width, heads, batch, kind)


@pytest.mark.parametrize("tokens,width,heads,batch,kind", _cases(adc.F32_TOKENS, adc.f32_shapes))
def test_attention_f32_vs_float64(tokens, width, heads, batch, kind):
    """mpreid_vit_attention_f32: attention_f32_kernel up to 320 tokens, attention_f32_chunked_kernel above -- the rule
    mpreid_vit_forward_f32 runs in every block"""
    run_case("fp32", tokens, width, heads, batch, kind)


# ---- the persistent loop of every resident instantiation, wrapped ------------------------------------------------------------
def _cus():
    from mpreid import _lib
    cus = C.c_int(0)
    _lib.require_gpu()
    _lib.check(_lib.load().mpreid_device_info(None, 0, C.byref(cus), None), "mpreid_device_info")
    assert cus.value > 0
    return cus.value


@pytest.mark.parametrize("tokens", adc.FORMS_ROWS)
@pytest.mark.parametrize("prec", ["fp16", "split"])
def test_wrapped_persistent_loop_gives_the_bits_of_a_batch_of_8(prec, tokens):
    """Eight distinct slabs repeated until B * heads exceeds the largest persistent grid (16 workgroups per CU up to 32 tokens, 4
    above: the figures of test_persistent_loop_wraps_with_the_same_bits), so that every workgroup walks several (image, head) pairs
    with the next pair's K / V prefetched into registers: the rows of every repetition are those of the batch of 8, bit for bit,
    and those are within the bound"""
    width, heads = 128, 2
    per_cu = 16 if tokens <= 32 else 4
    reps = (_cus() * per_cu // heads) // 8 + 1
    batch = 8 * reps
    assert batch * heads > _cus() * per_cu
    host, want, scale, _ = reference(prec, tokens, width, heads, 8, "plain")
    qkv = host.cuda()
    got, base = adc.checked_call(qkv, 8, tokens, heads, tag=(prec, tokens, "batch of 8"))
    err = adc.error_figure(got, want, scale)
    print("ATTFORMS wrap prec=%s L=%d B=%d err=%.3e" % (prec, tokens, batch, err))
    assert err <= BOUND[prec] and not torch.equal(base[0], base[1])
    big = qkv.view(8, tokens, -1).repeat(reps, 1, 1).view(batch * tokens, -1).contiguous()
    for run in range(2):
        bits = adc.guarded_call(big, batch, tokens, heads)[1].view(reps, 8, tokens, -1)
        differ = (bits != base[None]).any(-1).any(-1).nonzero()
        assert differ.numel() == 0, (prec, tokens, run, batch, "[repetition, image]", differ[:8].tolist())


# ---- the comparator bites at every form's own output ----------------------------------------------------------------------------
@pytest.mark.parametrize("prec,tokens", [(p, t) for p in ("fp16", "split") for t in adc.FORMS_ROWS + [257]]
                         + [("fp32", 129), ("fp32", 321)])
def test_swapped_value_rows_are_caught(prec, tokens):
    """one L per instantiation, the spiked LAST key: the kernel runs on operands whose v rows L - 1 and L - 2 are swapped -- a
    moved key, as a kernel with an off-by-one in its P V step would see it -- and its figure against the reference of the
    UNSWAPPED operands is at least 25 times the bound of that form"""
    width, heads, batch = 128, 2, 3
    host, want, scale, _ = reference(prec, tokens, width, heads, batch, "spike%d" % (tokens - 1))
    moved = host.clone().view(batch, tokens, 3, width)
    moved[:, [tokens - 1, tokens - 2], 2] = moved[:, [tokens - 2, tokens - 1], 2]
    got, _ = adc.checked_call(moved.view(batch * tokens, 3 * width).cuda(), batch, tokens, heads, f32=prec == "fp32",
                              tag=(prec, tokens, "swapped"))
    err = adc.error_figure(got, want, scale)
    print("ATTFORMS swapped prec=%s L=%d err=%.3e (25 x bound = %.3e)" % (prec, tokens, err, 25.0 * BOUND[prec]))
    assert err >= 25.0 * BOUND[prec]
