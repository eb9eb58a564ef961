"""GPU: the fused FP64 DCT pair reads and writes the public u64 ciphertexts 16 bytes per lane (csrc/dct_fused.hip, the
paired pass-0 layout: a thread carries two neighbouring columns of two polynomials through pass 0 instead of one column of
four).  Every case is compared bit for bit with the library's general three-launch u64 path (FHE_DCT_FORCE_U64=1), which
shares no kernel, layout or table with the fused pair.

The placement ramp gives every word of a block its own value, (i * 128 + 2 c + s) mod q for coefficient i of ciphertext c,
polynomial s: a swapped column pair, a swapped polynomial half or a misrouted row of the new exchanges changes the result."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

T = 1 << 14
Q36 = [0xFFFF00001, 0xFFFE58001, 0xFFFCB8001]              # <= 37 bits: packed intermediate
Q40 = [0xFFFFE80001, 0x7FFFFB0001, 0x7FFFE60001]           # 39/40 bits: FP64 intermediate
Q46 = [0x3FFFFFF70001, 0x7FFFFFFC8001, 0xFFFFFDF8001]      # 44..47 bits: BIG
P4096 = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]           # the headline preset

CONTEXTS = {
    "n2048-36b": (2048, Q36, {}),                          # <11,3>: 128-thread halves, the smallest paired shape
    "P4096": (4096, P4096, {}),                            # packed intermediate
    "P4096-pack0": (4096, P4096, {"FHE_DCT_PACK": 0}),     # FP64 intermediate
    "P4096-ldsc0": (4096, P4096, {"FHE_DCT_LDSC": 0}),     # row constants through registers
    "n4096-40b": (4096, Q40, {}),                          # FP64 intermediate
    "n4096-46b": (4096, Q46, {}),                          # BIG
    "n8192-36b": (8192, Q36, {}),                          # <13,3>
    "n1024-36b": (1024, Q36, {}),                          # <10,4>: keeps the 8-byte bodies
}
PATTERNS = ["random", "all-q-1", "ramp", "ramp-reversed"]


def _contexts(fhe, n, q, switches):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = fhe.SEALContext(n, q, T, switches=dict(switches, FHE_DCT_WAVE_BLOCKS=2))
    ref = fhe.SEALContext(n, q, T, switches={"FHE_DCT_FORCE_U64": 1})
    assert fhe._lib.call("fhe_dct_path", ctx.h) == 1, "the context under test must take the fused FP64 pair"
    assert fhe._lib.call("fhe_dct_path", ref.h) == 0, "the reference context must take the general u64 path"
    return ctx, ref


def _pattern(ctx, name, n_blocks):
    """[n_blocks, 64, 2, k, n]; ciphertext 8 * row + col of a block"""
    import torch
    if name == "random":
        return ctx.random_ct(n_blocks, 64, seed=777 + n_blocks)
    qs = torch.tensor(list(ctx.q), dtype=torch.int64, device=ctx.device).view(1, 1, 1, ctx.k, 1)
    out = ctx.empty(n_blocks, 64)
    if name == "all-q-1":
        out[:] = qs - 1
        return out
    n = out.shape[-1]
    i = torch.arange(n, dtype=torch.int64, device=ctx.device)
    if name == "ramp-reversed":
        i = n - 1 - i
    c = torch.arange(64, dtype=torch.int64, device=ctx.device).view(1, 64, 1, 1, 1)
    s = torch.arange(2, dtype=torch.int64, device=ctx.device).view(1, 1, 2, 1, 1)
    out[:] = (i.view(1, 1, 1, 1, n) * 128 + 2 * c + s) % qs
    return out


def _dct(fhe, ctx, blocks):
    return fhe.Evaluator(ctx).dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blocks)


def test_the_ramp_gives_every_word_of_a_block_its_own_value(fhe):
    import torch
    n, q, switches = CONTEXTS["n2048-36b"]
    ctx, _ = _contexts(fhe, n, q, switches)
    for pat in ("ramp", "ramp-reversed"):
        ramp = _pattern(ctx, pat, 1)
        for prime in range(ctx.k):
            assert torch.unique(ramp[0, :, :, prime, :]).numel() == 64 * 2 * n


@pytest.mark.parametrize("n_blocks", [1, 3])
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_public_wide_variants_match_the_general_path(fhe, name, n_blocks):
    """every shape the paired layout touches (and n = 1024, which must not take it), 1 block and 3 blocks in waves of 2"""
    import torch
    n, q, switches = CONTEXTS[name]
    ctx, ref = _contexts(fhe, n, q, switches)
    ev, plan = fhe.Evaluator(ctx), fhe.DctPlan(ctx, fhe.YQT)
    ev_ref, plan_ref = fhe.Evaluator(ref), fhe.DctPlan(ref, fhe.YQT)
    for pat in PATTERNS:
        blocks = _pattern(ctx, pat, n_blocks)
        got = ev.dct8x8_quant(plan, blocks)
        want = ev_ref.dct8x8_quant(plan_ref, blocks)
        torch.cuda.synchronize()
        assert torch.equal(got, want), "pattern %s" % pat


def test_repeated_launches_store_what_they_computed(fhe):
    """The wide output stores of a thread share one register quadruple; without wait states behind each store (gst_u64x2,
    csrc/fp64_core.h) a store picked up the next value in four lanes of one wave about once in 90 launches of 64 blocks, in
    any variant.  400 launches: a build without the wait states passes this with a probability of about 1 %."""
    import torch
    n, q, switches = CONTEXTS["P4096"]
    ctx = fhe.SEALContext(n, q, T)
    ref = fhe.SEALContext(n, q, T, switches={"FHE_DCT_FORCE_U64": 1})
    ev, plan = fhe.Evaluator(ctx), fhe.DctPlan(ctx, fhe.YQT)
    blocks = ctx.random_ct(64, 64, seed=123)
    want = _dct(fhe, ref, blocks)
    bad = 0
    for _ in range(400):
        bad += int(not torch.equal(ev.dct8x8_quant(plan, blocks), want))
    assert bad == 0, "%d of 400 launches differ from the general path" % bad


@pytest.mark.parametrize("name", ["P4096", "n2048-36b"])
def test_the_8_byte_switch_gives_the_same_bits(fhe, name):
    """FHE_DCT_WIDE_IO=0 selects the 8-byte bodies everywhere"""
    import torch
    n, q, switches = CONTEXTS[name]
    ctx, ref = _contexts(fhe, n, q, switches)
    narrow, _ = _contexts(fhe, n, q, dict(switches, FHE_DCT_WIDE_IO=0))
    for pat in PATTERNS:
        blocks = _pattern(ctx, pat, 3)
        wide, eight, want = _dct(fhe, ctx, blocks), _dct(fhe, narrow, blocks), _dct(fhe, ref, blocks)
        torch.cuda.synchronize()
        assert torch.equal(wide, eight), "pattern %s" % pat
        assert torch.equal(eight, want), "pattern %s" % pat


@pytest.mark.parametrize("name", ["P4096", "n2048-36b"])
def test_inputs_and_outputs_that_are_8_but_not_16_byte_aligned(fhe, name):
    """the C ABI promises 8-byte alignment only: `in`, `out` or both 8 bytes into a larger buffer give the bits of the aligned
    call, and the words of out's buffer around the result keep their fill value"""
    import torch
    n, q, switches = CONTEXTS[name]
    ctx, ref = _contexts(fhe, n, q, switches)
    plan = fhe.DctPlan(ctx, fhe.YQT)
    n_blocks, fill = 3, 5
    blocks = _pattern(ctx, "ramp", n_blocks)
    want = _dct(fhe, ref, blocks)
    words = blocks.numel()
    nbytes = int(fhe._lib.load().fhe_dct8x8_scratch_bytes(ctx.h, n_blocks))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
    src = torch.zeros(words + 2, dtype=torch.int64, device=ctx.device)
    assert src.data_ptr() % 16 == 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for in_shift, out_shift in ((0, 0), (1, 0), (0, 1), (1, 1)):
        src.zero_()
        src[in_shift:in_shift + words] = blocks.reshape(-1)
        dst = torch.full((words + 2,), fill, dtype=torch.int64, device=ctx.device)
        assert dst.data_ptr() % 16 == 0
        fhe._lib.call("fhe_dct8x8_quant", ctx.h, plan.h, C.c_void_p(src.data_ptr() + 8 * in_shift), C.c_void_p(dst.data_ptr() + 8 * out_shift), n_blocks,
                      C.c_void_p(scratch.data_ptr()), nbytes, stream)
        torch.cuda.synchronize()
        where = "in + %d, out + %d bytes" % (8 * in_shift, 8 * out_shift)
        assert torch.equal(dst[out_shift:out_shift + words].view_as(want), want), where
        outside = torch.cat([dst[:out_shift], dst[out_shift + words:]])
        assert bool((outside == fill).all()), where
