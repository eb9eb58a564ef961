"""GPU: the fused FP64 DCT pair addresses its tensors through per-workgroup windows (a 64-bit uniform base in a buffer
descriptor + 32-bit offsets, csrc/fp64_core.h gwin).  The cases below are the ones such addressing can break; each is
compared bit for bit with the library's own general three-launch u64 path (FHE_DCT_FORCE_U64=1, the switch
test_dct_variants_give_the_same_bits' neighbours use), which shares no kernel and no addressing with the fused pair.

Word offsets beyond 2^32 from the tensor start are covered by tests/test_gpu_parity.py and tests/test_gpu_sharding.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 1 << 14
# primes = 1 (mod 32768): NTT-friendly for every n <= 16384.  Three per size class of the fused pair:
Q36 = [0xFFFF00001, 0xFFFE58001, 0xFFFCB8001]              # <= 37 bits: packed intermediate
Q40 = [0xFFFFE80001, 0x7FFFFB0001, 0x7FFFE60001]           # 39/40 bits: FP64 intermediate
Q46 = [0x3FFFFFF70001, 0x7FFFFFFC8001, 0xFFFFFDF8001]      # 44..47 bits: BIG (reductions between the inverse passes)
P4096 = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]           # the headline preset


def _contexts(fhe, n, q, **switches):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = fhe.SEALContext(n, q, T, switches=switches) if switches else fhe.SEALContext(n, q, T)
    ref = fhe.SEALContext(n, q, T, switches={"FHE_DCT_FORCE_U64": 1})
    assert fhe._lib.call("fhe_dct_path", ctx.h) == 1, "the context under test must take the fused FP64 pair"
    assert fhe._lib.call("fhe_dct_path", ref.h) == 0, "the reference context must take the general u64 path"
    return ctx, ref


def _dct(fhe, ctx, blocks, out=None):
    ev, plan = fhe.Evaluator(ctx), fhe.DctPlan(ctx, fhe.YQT)
    return ev.dct8x8_quant(plan, blocks) if out is None else ev.dct8x8_quant(plan, blocks, out=out)


@pytest.mark.parametrize("n,q", [(4096, P4096), (2048, Q36), (8192, Q36), (2048, Q40), (4096, Q40), (8192, Q40), (2048, Q46), (4096, Q46), (8192, Q46)],
                         ids=["P4096", "n2048-36b", "n8192-36b", "n2048-40b", "n4096-40b", "n8192-40b", "n2048-46b", "n4096-46b", "n8192-46b"])
def test_every_body_variant_matches_the_general_path_on_sliced_tensors(fhe, n, q):
    """packed / FP64 intermediate / BIG bodies at n = 2048, 4096, 8192; input and output are slices of larger tensors that
    start at block 2 (a non-zero storage offset), 5 blocks in waves of 2 (FHE_DCT_WAVE_BLOCKS: a ragged last wave and a
    window base that moves with the wave); the blocks around the output slice must stay untouched"""
    import torch
    ctx, ref = _contexts(fhe, n, q, FHE_DCT_WAVE_BLOCKS=2)
    store = ctx.random_ct(9, 64, seed=1000 + n)
    blocks = store[2:7]
    assert blocks.storage_offset() != 0 and blocks.is_contiguous()
    want = _dct(fhe, ref, blocks.clone())
    got_new = _dct(fhe, ctx, blocks)
    assert torch.equal(got_new, want)
    canvas = torch.full_like(store, 7)
    view = canvas[3:8]
    got = _dct(fhe, ctx, blocks, out=view)
    torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr()
    assert torch.equal(view, want)
    assert bool((canvas[:3] == 7).all()) and bool((canvas[8:] == 7).all())


def test_block_count_ragged_against_the_256_block_wave(fhe):
    """258 blocks of the headline preset with the default wave of 256: the second wave holds 2 blocks and starts 256 blocks
    (3 GiB) into the input and output; compared on the device with the general path"""
    import torch
    ctx, ref = _contexts(fhe, 4096, P4096)
    blocks = ctx.random_ct(258, 64, seed=77)
    got = _dct(fhe, ctx, blocks)
    want = _dct(fhe, ref, blocks)
    torch.cuda.synchronize()
    assert torch.equal(got[256:], want[256:])
    assert torch.equal(got[:256], want[:256])


def test_packed_pair_matches_the_oracle_from_a_slice(fhe, oracle_mod):
    """one anchor outside the library: the headline instantiation on a sliced input against the CPU oracle"""
    ctx = fhe.SEALContext(4096, P4096, T)
    orc = oracle_mod.Oracle(4096, P4096, T)
    store = ctx.random_ct(4, 64, seed=31)
    got = fhe.to_host(_dct(fhe, ctx, store[1:4]))
    assert np.array_equal(got[2], orc.dct_quant(fhe.to_host(store)[3], fhe.YQT))
