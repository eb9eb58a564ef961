"""CPU: the slot model of the fused FP64 DCT / IDCT pair (tests/slot_craft.py) equals the CPU oracle, and the inputs crafted with
it reach -- in the exact model, as conditions and not as tolerances -- the residues and magnitudes they are aimed at.
tests/test_gpu_dct_slot_extremes.py runs those inputs through the kernels.

Run with -s for the table: per GPU context the worst-case sum that the unreduced inverse transform carries (F4) against 2^53,
the number of slots the solver left out, and the extreme high bytes that F1 sends through the packed intermediate."""
import numpy as np
import pytest

import idct_oracle as io
import slot_craft as sc
from test_dct_pack_format import _bias, _pack, _unpack

CPU_CONTEXTS = {"n1024-P4096": (1024, sc.P4096), "n2048-40b": (2048, sc.Q40), "n1024-46b": (1024, sc.Q46)}


@pytest.fixture(scope="module")
def crafted(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            n, q = CPU_CONTEXTS[name]
            orc = oracle_mod.Oracle(n, q, sc.T)
            m = sc.SlotModel(orc, oracle_mod.YQT)
            cache[name] = (orc, m, {d: sc.craft_batch(m, d, n == 1024) for d in ("fwd", "inv")})
        return cache[name]
    return get


def _p(m):
    return m.Pi.reshape(m.k, 1)


def test_modular_arithmetic_matches_python_integers(oracle_mod):
    rng = np.random.default_rng(1)
    for q in (sc.P4096, sc.Q40, sc.THRESHOLD_SETS["above47"]):
        m = sc.SlotModel(oracle_mod.Oracle(1024, q, sc.T), oracle_mod.YQT)
        a = rng.integers(0, 1 << 62, size=(m.k, m.n), dtype=np.int64).astype(np.uint64) % m.P
        b = rng.integers(0, 1 << 62, size=(m.k, m.n), dtype=np.int64).astype(np.uint64) % m.P
        a[:, 0], b[:, 0], a[:, 1], b[:, 1] = m.P[:, 0] - np.uint64(1), m.P[:, 0] - np.uint64(1), m.H[:, 0], m.H[:, 0] + np.uint64(1)
        prod, (inv, nz) = m.mul(a, b), m.inv(a)
        for i, p in enumerate(q):
            assert [int(x) for x in prod[i]] == [int(x) * int(y) % p for x, y in zip(a[i], b[i])]
            assert all(int(x) * int(y) % p == 1 for x, y, z in zip(a[i], inv[i], nz[i]) if z)
        assert np.array_equal(m.res(m.centre(a)), a) and np.abs(m.centre(a)).max() <= m.H.max()


def test_threshold_primes_are_what_the_search_finds():
    assert sc.search_prime(1 << 37, +1) == sc.P_ABOVE_37 and sc.P_ABOVE_37.bit_length() == 38
    assert sc.search_prime(1 << 40, +1) == sc.P_ABOVE_40 and sc.P_ABOVE_40.bit_length() == 41
    assert sc.search_prime(1 << 47, -1) == sc.P_BELOW_47 and sc.P_BELOW_47.bit_length() == 47
    assert sc.search_prime(1 << 47, +1) == sc.P_ABOVE_47 and sc.P_ABOVE_47.bit_length() == 48
    for q in [sc.Q36, sc.Q40, sc.Q46] + list(sc.THRESHOLD_SETS.values()):           # NTT primes up to n = 8192
        assert all(sc.is_prime(p) and p % (1 << 14) == 1 for p in q) and len(set(q)) == len(q)
    assert all(sc.is_prime(p) and p % (1 << 13) == 1 for p in sc.P4096)                # the headline primes: up to n = 4096


@pytest.mark.parametrize("direction", ["fwd", "inv"])
@pytest.mark.parametrize("name", list(CPU_CONTEXTS))
def test_model_agrees_with_the_oracle(crafted, oracle_mod, name, direction):
    """on every crafted block, the alternating-ties block and a random one: the model's residues at the input of the inverse
    transform are the forward transform of the oracle's output ciphertexts"""
    orc, m, batches = crafted(name)
    names, blocks, _, _ = batches[direction]
    todo = [(nm, blocks[i]) for i, nm in enumerate(names) if not nm.startswith("F2") or nm == "F2-ties"]
    if direction == "inv":
        todo.append(("random", orc.random_ct(64, seed=77)))
    for nm, block in todo:
        if direction == "fwd":
            want, got = orc.dct_quant(block, oracle_mod.YQT), m.forward(m.to_slots(block))["final"]
        else:
            want, got = io.OracleOps(orc).idct_block(block, oracle_mod.YQT), m.inverse(m.to_slots(block))["final"]
        assert np.array_equal(m.to_slots(want), got), nm


@pytest.mark.parametrize("name", list(CPU_CONTEXTS))
def test_f1_forward_rows_store_the_extremes(crafted, name):
    """row r: odd output {1,3,5,7}[r % 4] is exactly s (2p - 2), output 2 (r even) or 6 (r odd) s (p - 1); outputs 0 and 4 are
    congruent to +-s (p - 1) / 2 and so leave the packed variant's reduction as the tie residues +-(p - 1) / 2 (a reduced value
    cannot be larger); polynomial 1 carries the opposite signs.  Every product behind them is +-(p - 1) / 2."""
    orc, m, batches = crafted(name)
    names, blocks, _, _ = batches["fwd"]
    mod = m.forward(m.to_slots(blocks[names.index("F1")]))
    st, p = mod["stored"], _p(m)
    for r in range(8):
        s = 1 if r < 4 else -1
        for poly, sg in ((0, s), (1, -s)):
            o = sc.FWD_ODD_OUTPUTS[r % 4]
            assert (st[r, o, poly] == sg * (2 * p - 2)).all()
            assert (st[r, 6 if r % 2 else 2, poly] == sg * (p - 1)).all()
            assert (st[r, 0, poly] == sg * (p - 1) // 2).all() and (st[r, 4, poly] == -sg * (p - 1) // 2).all()
            for term in sc.FWD_ODD.out[o] + sc.FWD_EVEN.out[6 if r % 2 else 2]:
                assert (mod["row_products"][term[1]][r, poly] == sg * (p - 1) // 2).all()
    assert (st == 2 * p - 2).any() and (st == -(2 * p - 2)).any()
    if max(q.bit_length() for q in m.q) <= 37:      # the packed format: both extreme high bytes occur and survive pack / unpack
        for i, q in enumerate(m.q):
            v = st[..., i, :].reshape(-1)
            assert {(2 * q - 2) >> 32, (-(2 * q - 2)) >> 32} <= set(np.unique(v >> 32).tolist())
            lo, _, byte = _pack(v, _bias())
            assert np.array_equal((_unpack(lo, byte) - _bias()).astype(np.int64), v)


@pytest.mark.parametrize("name", list(CPU_CONTEXTS))
def test_f1_inverse_rows_reach_two_p_before_the_reduction(crafted, name):
    """row r: the four products of O[r % 4] are s (p - 1) / 2, O is s (2p - 2) before its reduction; the scaled d0 is s (p - 1) / 2
    and t3 (r even) or t2 (r odd) is s (p - 1), which takes E0 or E1 to s (2p - 2)"""
    orc, m, batches = crafted(name)
    names, blocks, _, _ = batches["inv"]
    mod = m.inverse(m.to_slots(blocks[names.index("F1")]))
    p = _p(m)
    for r in range(8):
        s = 1 if r < 4 else -1
        for poly, sg in ((0, s), (1, -s)):
            assert (mod["O_pre"][r, r % 4, poly] == sg * (2 * p - 2)).all()
            assert (mod["E_pre"][r, r % 2, poly] == sg * (2 * p - 2)).all()
            assert (mod["scaled"][r, 0, poly] == sg * (p - 1) // 2).all()
            for term in sc.INV_ODD.out[r % 4] + [(1, "e0"), (1, "e1" if r % 2 else "e2")]:
                assert (mod["row_products"][term[1]][r, poly] == sg * (p - 1) // 2).all()


@pytest.mark.parametrize("name", list(CPU_CONTEXTS))
def test_f3_column_operands_reach_their_bound(crafted, name):
    """forward: the scale product of column c's odd output {1,3,5,7}[c % 4] is given s (2p - 2).  inverse: every stored E and O is
    (p - 1) / 2 in magnitude, the column inputs E +- O are +-(p - 1) or 0, and z3 + z4 is +-4 (p - 1): the documented largest operand"""
    orc, m, batches = crafted(name)
    p = _p(m)
    names, blocks, _, _ = batches["fwd"]
    mod = m.forward(m.to_slots(blocks[names.index("F3")]))
    for c in range(8):
        s = 1 if c < 4 else -1
        for poly, sg in ((0, s), (1, -s)):
            assert (mod["operand"][sc.FWD_ODD_OUTPUTS[c % 4], c, poly] == sg * (2 * p - 2)).all()
    names, blocks, _, _ = batches["inv"]
    for nm, cols in (("F3", range(0, 4)), ("F3-diff", range(4, 8))):
        mod = m.inverse(m.to_slots(blocks[names.index(nm)]))
        assert (np.abs(mod["E"]) == (p - 1) // 2).all() and (np.abs(mod["O"]) == (p - 1) // 2).all()
        for c in range(8):
            for poly, sg in ((0, 1), (1, -1)):
                want = sg * (p - 1) if c in cols else 0 * p
                assert (mod["col_in"][:, c, poly] == want).all()
                assert (mod["col_operands"]["z5"][c, poly] == 4 * want).all()


@pytest.mark.parametrize("direction", ["fwd", "inv"])
@pytest.mark.parametrize("name", list(CPU_CONTEXTS))
def test_f4_hands_the_inverse_transform_the_pattern(crafted, name, direction):
    """the residues at the input of the inverse transform are exactly G (polynomial 1: -G); the all-plus pattern sums to
    n (p - 1) / 2 over the slots, which is what one element of the unreduced X + Y chain carries"""
    orc, m, batches = crafted(name)
    names, blocks, G, pats = batches[direction]
    S = m.to_slots(blocks[names.index("F4")])
    final = (m.forward(S) if direction == "fwd" else m.inverse(S))["final"]
    assert np.array_equal(final[:, :, 0], G) and np.array_equal(final[:, :, 1], m.neg(G))
    assert pats[0] is None and pats[1:] == m.f4_bits(m.n == 1024)
    plus = m.centre(final[0, 0, 0])
    assert [int(x) for x in plus.sum(axis=-1)] == [m.n * (q - 1) // 2 for q in m.q]
    one = m.centre(final[0, 1, 0])                      # pattern of bit 0: half the slots each sign
    assert (np.abs(one) == (_p(m) - 1) // 2).all() and (one.sum(axis=-1) == 0).all()


def _unique_gpu_contexts():
    seen = {}
    for name, (n, q, _, fused) in sc.GPU_CONTEXTS.items():
        seen.setdefault((n, tuple(q)), (name, fused))
    return [(name, n, list(q), fused) for (n, q), (name, fused) in seen.items()]


@pytest.mark.parametrize("name,n,q,fused", _unique_gpu_contexts(), ids=[c[0] for c in _unique_gpu_contexts()])
def test_every_gpu_context_has_headroom_and_no_slot_left_out(oracle_mod, name, n, q, fused):
    """per (n, primes) of the GPU file, one table row: n (p - 1) / 2 for the largest prime against 2^53 -- asserted below 2^53
    wherever the inverse transform does not reduce between its passes (primes of at most 40 bits); the solver's left-out count
    with its 1 % cap; for primes of at most 37 bits the extreme high bytes that F1's row outputs put into the packed intermediate"""
    bits, worst = max(p.bit_length() for p in q), n * (max(q) - 1) // 2
    m = sc.SlotModel(oracle_mod.Oracle(n, q, sc.T), oracle_mod.YQT)
    bad = m.solver_left_out()
    high = "-"
    if bits <= 37:
        st = m.forward(m.craft_fwd_f1()[0][:, :, None])["stored"]
        hb = sorted(set(np.unique(st >> 32).tolist()))
        assert all(-128 <= b <= 127 for b in hb)
        for p in q:
            assert (2 * p - 2) >> 32 in hb and (-(2 * p - 2)) >> 32 in hb
        high = "%d .. %d" % (hb[0], hb[-1])
    print("\n%-14s n %4d  max bits %2d  n (p-1)/2 = %18d = %8.5f x 2^53  left out %d of %d  F1 high bytes %s"
          % (name, n, bits, worst, worst / 2.0 ** 53, bad, m.k * m.n, high))
    assert bad <= sc.MAX_LEFT_OUT * m.k * m.n
    if fused and bits <= 40:
        assert worst < 1 << 53
