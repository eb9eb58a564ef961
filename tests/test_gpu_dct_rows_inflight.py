"""GPU: the wide row kernel of the fused FP64 DCT pair keeps three groups of input requests in flight (csrc/dct_fused.hip,
rows_body, WIDE): the `a` side of a thread's 16 pairs d_m +- d_(7-m) lands in the registers that become x, the `b` side goes
through a ring of eight register quadruples, and b(8+i) is requested into the slot of b(i) as soon as pair i is formed.
Every case is compared bit for bit with the library's general three-launch u64 path (FHE_DCT_FORCE_U64=1).

Patterns, per row of eight ciphertexts m = 0..7 (a thread's `a` requests read m = 0..3, its `b` requests m = 4..7):
  ramp-b   m = 0..3 hold C0 everywhere, m = 4..7 hold (i * 8 + (7 - m)) mod q at coefficient i: each of the 16 `b` requests of a
           thread carries its own value, so a ring slot reused too early or paired with the wrong `a` changes the result
  ramp-a   the mirror image: m = 0..3 hold (i * 8 + m) mod q, m = 4..7 hold C0
  all-q-1  the largest residue everywhere
One block already runs both halves, both polynomials, every prime and all eight lines; the headline preset takes 2 blocks."""
import pytest

pytestmark = pytest.mark.gpu

T = 1 << 14
C0 = 0x123456789                                            # below every prime used here
Q36 = [0xFFFF00001, 0xFFFE58001, 0xFFFCB8001]               # <= 37 bits: packed intermediate
P4096 = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]            # the headline preset

CONTEXTS = {                                                # name: (n, primes, switches, blocks)
    "n2048-36b": (2048, Q36, {}, 1),                        # <11,3>: the smallest wide shape
    "P4096": (4096, P4096, {}, 2),                          # <12,3>, packed intermediate, constants through LDS: the headline kernel
    "P4096-pack0": (4096, P4096, {"FHE_DCT_PACK": 0}, 1),   # FP64 intermediate
    "P4096-ldsc0": (4096, P4096, {"FHE_DCT_LDSC": 0}, 1),   # row constants through registers
    "n8192-36b": (8192, Q36, {}, 1),                        # <13,3>
}
PATTERNS = ["ramp-b", "ramp-a", "all-q-1"]


def _contexts(fhe, n, q, switches):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = fhe.SEALContext(n, q, T, switches=dict(switches, FHE_DCT_WAVE_BLOCKS=2))
    ref = fhe.SEALContext(n, q, T, switches={"FHE_DCT_FORCE_U64": 1})
    assert fhe._lib.call("fhe_dct_path", ctx.h) == 1, "the context under test must take the fused FP64 pair"
    assert fhe._lib.call("fhe_dct_path", ref.h) == 0, "the reference context must take the general u64 path"
    return ctx, ref


def _pattern(ctx, name, n_blocks):
    """[n_blocks, 64, 2, k, n]; ciphertext 8 * row + m of a block"""
    import torch
    qs = torch.tensor(list(ctx.q), dtype=torch.int64, device=ctx.device).view(1, 1, 1, ctx.k, 1)
    out = ctx.empty(n_blocks, 64)
    if name == "all-q-1":
        out[:] = qs - 1
        return out
    n = out.shape[-1]
    i = torch.arange(n, dtype=torch.int64, device=ctx.device).view(1, 1, 1, 1, n)
    m = (torch.arange(64, dtype=torch.int64, device=ctx.device) % 8).view(1, 64, 1, 1, 1)
    if name == "ramp-b":
        ramp, ramped = (i * 8 + (7 - m)) % qs, m >= 4
    else:
        ramp, ramped = (i * 8 + m) % qs, m < 4
    out[:] = torch.where(ramped, ramp, torch.full_like(ramp, C0))
    return out


def test_each_request_of_a_thread_carries_its_own_value(fhe):
    """the ramped side of a row holds 4 * n different values per polynomial and prime, the other side C0 only"""
    import torch
    n, q, switches, _ = CONTEXTS["n2048-36b"]
    ctx, _ = _contexts(fhe, n, q, switches)
    for pat, ramped, flat in (("ramp-b", slice(4, 8), slice(0, 4)), ("ramp-a", slice(0, 4), slice(4, 8))):
        row = _pattern(ctx, pat, 1)[0, 8:16]
        assert int(row[flat].min()) == C0 and int(row[flat].max()) == C0
        for prime in range(ctx.k):
            assert torch.unique(row[ramped, 0, prime, :]).numel() == 4 * n


@pytest.mark.parametrize("pat", PATTERNS)
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_wide_row_variants_match_the_general_path(fhe, name, pat):
    import torch
    n, q, switches, n_blocks = CONTEXTS[name]
    ctx, ref = _contexts(fhe, n, q, switches)
    blocks = _pattern(ctx, pat, n_blocks)
    got = fhe.Evaluator(ctx).dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), blocks)
    want = fhe.Evaluator(ref).dct8x8_quant(fhe.DctPlan(ref, fhe.YQT), blocks)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_fifty_launches_on_the_same_inputs_agree(fhe):
    """a staging register overwritten while its request is in flight shows up rarely, not in every launch"""
    import torch
    n, q, switches, n_blocks = CONTEXTS["P4096"]
    ctx, ref = _contexts(fhe, n, q, switches)
    ev, plan = fhe.Evaluator(ctx), fhe.DctPlan(ctx, fhe.YQT)
    blocks = _pattern(ctx, "ramp-b", n_blocks)
    want = fhe.Evaluator(ref).dct8x8_quant(fhe.DctPlan(ref, fhe.YQT), blocks)
    bad = 0
    for _ in range(50):
        bad += int(not torch.equal(ev.dct8x8_quant(plan, blocks), want))
    assert bad == 0, "%d of 50 launches differ from the general path" % bad
