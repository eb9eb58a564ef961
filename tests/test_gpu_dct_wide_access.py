"""GPU: the fused FP64 DCT pair moves its private formats 16 bytes per lane -- the packed intermediate as two 16-byte planes
and one 8-byte plane of high bytes, the FP64 intermediate as planes of
value pairs, the column kernel's constants as paired tables.  Every case is compared bit for bit with the library's general
three-launch u64 path (FHE_DCT_FORCE_U64=1), which shares no kernel, layout or table with the fused pair.

Inputs beyond random residues are coefficient patterns of extreme residues (q - 1 or 0 by row and column), which take the
coefficient-side sums d_m + d_(7-m) and differences d_m - d_(7-m) to their largest magnitudes of either sign.  They do not
control what the row outputs hold: the row kernel transforms the polynomials first, and at the NTT slots these inputs behave
like random data.  The inputs that reach both ends of the packed range are built at the slots: tests/test_gpu_dct_slot_extremes.py."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

T = 1 << 14
Q36 = [0xFFFF00001, 0xFFFE58001, 0xFFFCB8001]              # <= 37 bits: packed intermediate
Q40 = [0xFFFFE80001, 0x7FFFFB0001, 0x7FFFE60001]           # 39/40 bits: FP64 intermediate
Q46 = [0x3FFFFFF70001, 0x7FFFFFFC8001, 0xFFFFFDF8001]      # 44..47 bits: BIG
P4096 = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]           # the headline preset

CONTEXTS = {
    "P4096": (4096, P4096, {}),
    "n2048-36b": (2048, Q36, {}),
    "n8192-36b": (8192, Q36, {}),
    "n4096-40b": (4096, Q40, {}),
    "n4096-46b": (4096, Q46, {}),
    "n1024-36b": (1024, Q36, {}),
    "P4096-pack0": (4096, P4096, {"FHE_DCT_PACK": 0}),
    "P4096-ldsc0": (4096, P4096, {"FHE_DCT_LDSC": 0}),
}
PATTERNS = ["random", "all-q-1", "all-0", "low-cols-q-1", "high-cols-q-1", "checkerboard"]


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
        return ctx.random_ct(n_blocks, 64, seed=4242 + n_blocks)
    top = torch.tensor([qi - 1 for qi in ctx.q], dtype=torch.int64, device=ctx.device).view(1, 1, 1, ctx.k, 1)
    row = torch.arange(64, device=ctx.device) // 8
    col = torch.arange(64, device=ctx.device) % 8
    mask = {"all-q-1": torch.ones(64, dtype=torch.bool, device=ctx.device), "all-0": torch.zeros(64, dtype=torch.bool, device=ctx.device),
            "low-cols-q-1": col < 4, "high-cols-q-1": col >= 4, "checkerboard": ((row + col) % 2) == 1}[name]
    out = ctx.empty(n_blocks, 64)
    out[:] = top * mask.view(1, 64, 1, 1, 1).to(torch.int64)
    return out


def _dct(fhe, ctx, blocks):
    return fhe.Evaluator(ctx).dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blocks)


@pytest.mark.parametrize("n_blocks", [1, 3])
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_wide_access_variants_match_the_general_path(fhe, name, n_blocks):
    """every body variant, 1 block and 3 blocks in waves of 2 (a ragged last wave), every input pattern"""
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


@pytest.mark.parametrize("name", ["P4096", "n4096-40b"])
def test_scratch_that_is_8_but_not_16_byte_aligned_gives_the_same_bits(fhe, name):
    """the C ABI with a scratch pointer 8 bytes into a larger buffer: the library rounds it up to the 16 bytes its wide
    accesses need, and fhe_dct8x8_scratch_bytes covers the bytes lost"""
    import torch
    n, q, switches = CONTEXTS[name]
    ctx, ref = _contexts(fhe, n, q, switches)
    plan = fhe.DctPlan(ctx, fhe.YQT)
    blocks = ctx.random_ct(3, 64, seed=99)
    want = _dct(fhe, ref, blocks)
    nbytes = int(fhe._lib.load().fhe_dct8x8_scratch_bytes(ctx.h, 3))
    buf = torch.empty(nbytes + 16, dtype=torch.uint8, device=ctx.device)
    assert buf.data_ptr() % 16 == 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for shift in (8, 0):
        out = torch.full_like(blocks, 5)
        fhe._lib.call("fhe_dct8x8_quant", ctx.h, plan.h, C.c_void_p(blocks.data_ptr()), C.c_void_p(out.data_ptr()), 3,
                      C.c_void_p(buf.data_ptr() + shift), nbytes, stream)
        torch.cuda.synchronize()
        assert torch.equal(out, want), "scratch offset %d" % shift


def test_bytes_lost_to_the_16_byte_round_up_are_counted(fhe):
    """a scratch of exactly one block's intermediate holds a block when it starts on a 16-byte boundary and none when it starts
    8 bytes off it (the library starts the intermediate at the next multiple of 16): the call is refused, not run short"""
    import torch
    n, q, switches = CONTEXTS["P4096"]
    ctx, ref = _contexts(fhe, n, q, switches)
    plan = fhe.DctPlan(ctx, fhe.YQT)
    blocks = ctx.random_ct(1, 64, seed=7)
    want = _dct(fhe, ref, blocks)
    one_block = blocks.numel() * 8                       # the FP64 intermediate of one block
    assert int(fhe._lib.load().fhe_dct8x8_scratch_bytes(ctx.h, 1)) == one_block + 16
    buf = torch.empty(one_block + 16, dtype=torch.uint8, device=ctx.device)
    assert buf.data_ptr() % 16 == 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.full_like(blocks, 5)
    args = (ctx.h, plan.h, C.c_void_p(blocks.data_ptr()), C.c_void_p(out.data_ptr()), 1)
    with pytest.raises(fhe._lib.FheError):
        fhe._lib.call("fhe_dct8x8_quant", *args, C.c_void_p(buf.data_ptr() + 8), one_block, stream)
    fhe._lib.call("fhe_dct8x8_quant", *args, C.c_void_p(buf.data_ptr()), one_block, stream)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
