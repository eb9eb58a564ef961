"""GPU: the fused u64 DCT pair (csrc/dct_u64.hip) at its arithmetic edges, in all fifteen kernel instantiations.  tests/dct_u64_craft.py
builds the inputs and restates the kernels as a value model; tests/test_dct_u64_craft_cpu.py proves in that model what the inputs reach
(the exits see 0 as q, 2q, 3q and q - 1 as 2q - 1, 3q - 1; the lazy ranges are measured against their static bounds).  Here the same blocks go
through the kernels.  Families, nine blocks per context:
  G  a random block, the all-(q - 1) block, the all-zero block
  Z  every ciphertext the same constant 1, (q - 1) / 2, (q + 1) / 2, q - 1: the DC output is 64 c encode(0.125) encode(1 / Q[0]), the other
     63 outputs are exactly zero -- through cancellation, so they reach the exits as multiples of q
  X  every coefficient of every output polynomial prescribed from {0, 1, 2, q/2, q/2 + 1, q - 2, q - 1} (the circuit inverted slot by slot)
  W  the block the model's search found to push the line_half sums and the inverse transform's differences furthest
Each batch runs in waves of two blocks (a ragged last wave, the intermediate buffer reused) and is compared bit for bit with the general
three-launch path, with the CPU oracle (every block at n = 2048, one per family above), with the closed form of Z and with the targets of X;
no output word is at or above its prime, the input is unchanged, and fhe_dct_path / fhe_arith_path report the class that
dct_u64_craft.classify -- the rule of fhe_dct_u64_launch restated -- expects.  A last case asserts that the contexts reached all nine row
and six column instantiations."""
import numpy as np
import pytest

import dct_u64_craft as dc

pytestmark = pytest.mark.gpu

FAMILIES = ("G", "Z", "X", "W")
ORACLE_ABOVE_2048 = ("G-random", "Z-half+", "X", "W")         # one block per family where n > 2048


def _grouped_contexts():
    """context names with those that share (n, primes) next to each other: their crafted batches are built once"""
    groups = {}
    for name, (n, q, _, _, _) in dc.CONTEXTS.items():
        groups.setdefault((n, tuple(q)), []).append(name)
    return [name for names in groups.values() for name in names]


@pytest.fixture(scope="module")
def runs(fhe, oracle_mod):
    """context -> the crafted batch, the fused pair's output, its comparison with the general path.  One batch (with its oracle outputs) and
    one run are kept at a time; the cases below are ordered to match.  `reached` collects (L, rows body, PM columns) of every context run."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    state = {"batch_key": None, "batch": None, "run_key": None, "run": None, "reached": {}}

    def get(name):
        if state["run_key"] == name:
            return state["run"]
        state["run"] = None
        n, q, t, switches, (body, pm) = dc.CONTEXTS[name]
        if state["batch_key"] != (n, tuple(q)):
            state["batch"] = None
            sm = dc.slot_model(oracle_mod, n, q, t)
            names, blocks, tg = dc.craft_batch(sm)
            want = {nm: sm.orc.dct_quant(blocks[b], oracle_mod.YQT) for b, nm in enumerate(names) if n == 2048 or nm in ORACLE_ABOVE_2048}
            state["batch_key"], state["batch"] = (n, tuple(q)), (sm, names, blocks, tg, want)
        sm, names, blocks, tg, want = state["batch"]
        ctx = fhe.SEALContext(n, q, t, switches=dict(switches, FHE_DCT_WAVE_BLOCKS=2))
        ref = fhe.SEALContext(n, q, t, switches=dict(switches, FHE_DCT_FORCE_U64=1))
        path, arith = fhe._lib.call("fhe_dct_path", ctx.h), fhe._lib.call("fhe_arith_path", ctx.h) & 3
        exp_path, exp_body, exp_pm, exp_arith = dc.classify(n, q, switches)
        assert (path, arith) == (exp_path, exp_arith) == (2, 1 if pm else arith), "%s: fhe_dct_path = %d, fhe_arith_path & 3 = %d" % (name, path, arith)
        assert (exp_body, exp_pm) == (body, pm) and (arith == 1) == pm
        assert fhe._lib.call("fhe_dct_path", ref.h) == 0, "the reference context must take the general three-launch path"
        dev = fhe.to_device(blocks, ctx.device)
        before = dev.clone()
        got = fhe.Evaluator(ctx).dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), dev)
        general = fhe.Evaluator(ref).dct8x8_quant(fhe.DctPlan(ref, fhe.YQT), dev)
        torch.cuda.synchronize()
        qv = torch.tensor(q, dtype=torch.int64, device=ctx.device).view(1, 1, 1, len(q), 1)
        state["reached"][name] = (n.bit_length() - 1, body, pm)
        state["run_key"] = name
        state["run"] = dict(quant=oracle_mod.YQT, sm=sm, names=names, tg=tg, want=want, n=n, q=q, got=fhe.to_host(got), untouched=bool(torch.equal(dev, before)),
                            same=[bool(torch.equal(got[b], general[b])) for b in range(len(names))],
                            unreduced=int(((got < 0) | (got >= qv)).sum()))
        return state["run"]
    get.state = state
    return get


@pytest.mark.parametrize("name,family", [(n, f) for n in _grouped_contexts() for f in FAMILIES])
def test_crafted_family_matches_the_oracle(runs, name, family):
    """family G also carries the whole-batch checks: every block bit-identical to the general path (which shares no kernel with the fused
    pair), no output word at or above its prime, the input unchanged"""
    run = runs(name)
    names, got, want, sm = run["names"], run["got"], run["want"], run["sm"]
    if family == "G":
        assert run["unreduced"] == 0 and run["untouched"]
        assert all(run["same"]), [nm for nm, ok in zip(names, run["same"]) if not ok]
        assert len(names) == 9
    mine = [b for b, nm in enumerate(names) if nm.split("-")[0] == family]
    assert mine and any(names[b] in want for b in mine)
    for b in mine:
        if names[b] in want:
            assert np.array_equal(got[b], want[names[b]]), names[b]
    if family == "G":
        assert not got[names.index("G-zero")].any()
    if family == "Z":
        for key in dc.Z_NAMES:
            out = got[names.index("Z-" + key)]
            assert np.array_equal(out, dc.z_expected(sm, key, run["quant"])) and not out[1:].any() and out[0].any(), key
    if family == "X":
        out, tg = got[names.index("X")], run["tg"]
        qv = np.array(run["q"], dtype=np.uint64).reshape(1, -1, 1)
        assert np.array_equal(out[:, 0], tg) and np.array_equal(out[:, 1], (qv - tg) % qv)


def test_all_fifteen_instantiations_were_reached(runs):
    """(L, LAZY, PM) of every context that ran above -- each asserted there against fhe_dct_path == 2 and fhe_arith_path -- cover
    k_dct_rows_u64<L, LAZY, PM> for the three bodies and k_dct_cols_u64<L, PM> for both, at L = 11, 12, 13.  PM is what the library reports;
    LAZY is inferred from the restated rule (56 bits at most), because the library has no query for it.  A context that no case above ran in
    this process (a -k selection, cases spread over workers) is run here first, with the same assertions on its path and class."""
    reached = runs.state["reached"]
    for name in dc.CONTEXTS:
        if name not in reached:
            runs(name)
    assert set(reached) == set(dc.CONTEXTS)
    got = set()
    for L, body, pm in reached.values():
        got.add(("rows", L, body != "nolazy", body == "pm"))
        got.add(("cols", L, pm))
    assert got == dc.ALL_INSTANTIATIONS and len(got) == 15
