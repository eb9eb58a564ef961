"""GPU: the fused FP64 DCT and IDCT pairs (csrc/dct_fused.hip) on inputs that are constructed at the NTT slots -- where the
kernels' products and reductions work -- so that the magnitude bounds their exactness rests on are reached, not merely
approached by random data.  tests/slot_craft.py builds the inputs from an exact integer model; tests/test_slot_craft_cpu.py
proves, in that model, that every family reaches what it is aimed at:
  F1  row products at +-(p - 1) / 2: the forward rows store +-(2p - 2) and +-(p - 1) (both ends of the packed range, the
      tie residues under the reduction of outputs 0 / 4); the inverse rows reduce O and E from +-(2p - 2)
  F2  every slot of every ciphertext holds 1, (p - 1) / 2, (p + 1) / 2 or p - 1 (and the two ties alternating): tie residues
      under the inverse rows' first reduction, d_m + d_(7-m) = p - 1, p, p + 1 in the forward rows
  F3  column operands: +-(2p - 2) into the forward scale products; E +- O = +-(p - 1) and z3 + z4 = +-4 (p - 1) in the
      inverse columns, once through the sums and once through the differences
  F4  the inverse transform's input is +(p - 1) / 2 at every slot, or +-(p - 1) / 2 by one bit of the slot index: the
      unreduced X + Y (X - Y) chain carries n (p - 1) / 2
Each batch of nine blocks runs through the fused pair in waves of two blocks (a ragged last wave) and is compared bit for bit
with the CPU oracle, with the library's general u64 path, with closed forms where there are any, and checked for reduced outputs.

Contexts: four sizes x three prime classes reach every launch_pair / launch_ipair case, switch variants the bodies no default
takes, and primes right next to each threshold (37, 40, 47 bits) the change of variant itself (slot_craft.GPU_CONTEXTS)."""
import numpy as np
import pytest

import idct_oracle as io
import slot_craft as sc

pytestmark = pytest.mark.gpu

FAMILIES = ("general", "F1", "F2", "F3", "F4")


def _grouped_contexts():
    """context names with those that share (n, primes) next to each other: their crafted batches are built once"""
    groups = {}
    for name, (n, q, _, _) in sc.GPU_CONTEXTS.items():
        groups.setdefault((n, tuple(q)), []).append(name)
    return [name for names in groups.values() for name in names]


RUNS = [(name, d) for name in _grouped_contexts() for d in ("fwd", "inv")]


@pytest.fixture(scope="module")
def runs(fhe, oracle_mod):
    """(context, direction) -> the crafted batch, the fused pair's output and the general path's, both on the host.  One model
    (with its crafted batches) and one run are kept at a time; the cases below are ordered to match."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    state = {"model_key": None, "model": None, "run_key": None, "run": None}

    def get(name, direction):
        if state["run_key"] == (name, direction):
            return state["run"]
        state["run"] = None
        n, q, switches, fused = sc.GPU_CONTEXTS[name]
        if state["model_key"] != (n, tuple(q)):
            orc = oracle_mod.Oracle(n, q, sc.T)
            state["model_key"], state["model"] = (n, tuple(q)), (orc, sc.SlotModel(orc, oracle_mod.YQT), {})
        orc, m, batches = state["model"]
        if direction not in batches:
            batches[direction] = sc.craft_batch(m, direction, every_bit=(n == 1024))
        names, blocks, G, pats = batches[direction]
        assert m.left_out == 0 or m.left_out <= sc.MAX_LEFT_OUT * m.crafted
        ctx = fhe.SEALContext(n, q, sc.T, switches=dict(switches, FHE_DCT_WAVE_BLOCKS=2))
        ref = fhe.SEALContext(n, q, sc.T, switches={"FHE_DCT_FORCE_U64": 1})
        path = fhe._lib.call("fhe_dct_path", ctx.h)
        assert (path == 1) == fused, "%s: fhe_dct_path = %d" % (name, path)
        assert fhe._lib.call("fhe_dct_path", ref.h) == 0, "the reference context must take the general u64 path"
        dev = fhe.to_device(blocks, ctx.device)
        if direction == "fwd":
            got = fhe.Evaluator(ctx).dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), dev)
            general = fhe.Evaluator(ref).dct8x8_quant(fhe.DctPlan(ref, fhe.YQT), dev)
        else:
            got = fhe.Evaluator(ctx).idct8x8_dequant(fhe.IdctPlan(ctx, fhe.YQT), dev)
            general = fhe.Evaluator(ref).idct8x8_dequant(fhe.IdctPlan(ref, fhe.YQT), dev)
        torch.cuda.synchronize()
        qv = torch.tensor(q, dtype=torch.int64, device=ctx.device).view(1, 1, 1, len(q), 1)
        state["run_key"] = (name, direction)
        state["run"] = dict(orc=orc, m=m, names=names, blocks=blocks, G=G, pats=pats, n=n, got=fhe.to_host(got),
                            same=[bool(torch.equal(got[b], general[b])) for b in range(len(names))],
                            unreduced=int(((got < 0) | (got >= qv)).sum()))
        return state["run"]
    return get


def _expect(run, oracle_mod, direction, b):
    if direction == "fwd":
        return run["orc"].dct_quant(run["blocks"][b], oracle_mod.YQT)
    return io.OracleOps(run["orc"]).idct_block(run["blocks"][b], oracle_mod.YQT)


@pytest.mark.parametrize("name,direction,family", [(n, d, f) for n, d in RUNS for f in FAMILIES])
def test_crafted_family_matches_the_oracle(runs, oracle_mod, name, direction, family):
    """family "general", all nine blocks: the same bits as the general u64 path, which shares no kernel, layout or table with the
    fused pair, and every output word below its prime -- a value outside (-p, p) at the final conversion shows up exactly there.
    Families F1 .. F4, bit for bit against the CPU oracle: every block of the family at n <= 2048, one per family above (F1, the alternating ties
    of F2, the first F3 block, F4).  Closed forms on top:
      F2 forward   a constant block has the DC output 64 c encode(0.125) encode(1 / Q[0]) and 63 zero ciphertexts
      F2 inverse   the circuit is linear, so the outputs of the constant blocks are c times the outputs of the block of ones
      F4           the residues at the slots of every output are the pattern G itself, and an all-plus output is the constant
                   polynomial (p - 1) / 2 (polynomial 1: (p + 1) / 2)"""
    run = runs(name, direction)
    if family == "general":
        assert run["unreduced"] == 0
        assert all(run["same"]), [nm for nm, ok in zip(run["names"], run["same"]) if not ok]
        return
    orc, m, names, got = run["orc"], run["m"], run["names"], run["got"]
    mine = [b for b, nm in enumerate(names) if nm.split("-")[0] == family]
    assert mine
    full = run["n"] <= 2048
    for b in mine:
        if full or names[b] in ("F1", "F2-ties", "F3", "F4"):
            assert np.array_equal(got[b], _expect(run, oracle_mod, direction, b)), names[b]
    if family == "F2":
        consts = m.f2_constants()
        one = got[names.index("F2-one")]
        for key in ("one", "half-", "half+", "top"):
            out, c = got[names.index("F2-" + key)], consts[key][0]
            if direction == "fwd":
                dc = np.zeros((2, m.k, m.n), dtype=np.uint64)
                for i, p in enumerate(m.q):
                    dc[0, i, 0], dc[1, i, 0] = 64 * c[i] % p, -64 * c[i] % p
                dc = orc.multiply_plain(orc.multiply_plain(dc, orc.encode(0.125)), orc.encode(1 / float(oracle_mod.YQT[0])))
                assert np.array_equal(out[0], dc) and not out[1:].any(), key
            else:
                assert np.array_equal(out, m.mul(m.full(c), one)), key
    if family == "F4":
        out = got[names.index("F4")]
        slots = m.to_slots(out)
        assert np.array_equal(slots[:, :, 0], run["G"]) and np.array_equal(slots[:, :, 1], m.neg(run["G"]))
        for i in range(0, 64, len(run["pats"])):                 # the all-plus outputs
            want = np.zeros((2, m.k, m.n), dtype=np.uint64)
            want[0, :, 0], want[1, :, 0] = m.H[:, 0], m.H[:, 0] + np.uint64(1)
            assert np.array_equal(out[i], want), i
