"""CPU: the specification of the diagonal linear maps on encrypted slots (tests/rotdiag_oracle.py) -- its residue form on the oracle's
transforms agrees with its big-integer form and with the structure the kernels use on every base the GPU tests use; constant plaintexts
reproduce tests/rotsum_oracle.py bit for bit; the identity drop(acc + p z) = drop(acc) + z on the crafted drop operands; a toy BFV
decrypts to sum_j d_j (.) rot_j(m) slot by slot within circuits.rotate_diag_budget; the wrong variants are caught; the host helpers
(packed_filter_diagonals, block_matvec_diagonals) against plain numpy; the refusals that need no device; the plan's host code under the
host sanitizers."""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo
import rotdiag_oracle as rd
import rotsum_oracle as rs
import test_keyswitch_sp_cpu as tk
import test_rotsum_cpu as tr

BASES = mo.bases(1024)
N_SMALL = 64
T = go.T_BATCH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plains(n, G, seed):
    """random dense, with the edge coefficients 0, 1, t - 1, (t - 1)/2, (t + 1)/2 in front; the last tap is (t - 1) X^(n-1)"""
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, T, size=n, dtype=np.uint64) for _ in range(G)]
    for p in out:
        p[:5] = [0, 1, T - 1, (T - 1) // 2, (T + 1) // 2]
    if G > 1:
        out[-1][:] = 0
        out[-1][n - 1] = T - 1
    return out


# ---- (a) the restatements agree --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BASES))
def test_residue_form_equals_the_big_integer_form(oracle_mod, name):
    q, n = BASES[name], N_SMALL
    elts = tr._taps5(n)
    orc, ct, kc, ko = tr._setup(oracle_mod, name, elts, seed=len(name) + 1)
    plains = _plains(n, len(elts), seed=len(name))
    for sel in ([0], [1], [0, 1], [0, 1, 2, 3, 4]):
        e, p = [elts[j] for j in sel], [plains[j] for j in sel]
        got = rd.rotate_diag_sum(orc, ct, T, e, p, [ko[j] for j in sel])
        assert np.array_equal(got, rd.rotate_diag_sum_big(q, T, ct, e, p, [kc[j] for j in sel])), (name, e)
        assert np.array_equal(got, rd.rotate_diag_sum_structured(orc, ct, T, e, p, [ko[j] for j in sel])), (name, e, "structured")
        for r in range(len(q) - 1):
            assert int(got[:, r].max()) < q[r]


@pytest.mark.parametrize("name", list(BASES))
def test_constant_plaintexts_reproduce_rotate_sum(oracle_mod, name):
    n = N_SMALL
    elts = tr._taps5(n)
    weights = rs.edge_weights(T) + [T - 7]
    orc, ct, _, ko = tr._setup(oracle_mod, name, elts, seed=3)
    for sel in ([0], [1], [0, 1, 2, 3, 4]):
        e, w = [elts[j] for j in sel], [weights[j] for j in sel]
        k = [ko[j] for j in sel]
        assert np.array_equal(rd.rotate_diag_sum(orc, ct, T, e, [rd.constant(n, x) for x in w], k), rs.rotate_sum(orc, ct, T, e, w, k)), (name, e)


# ---- (b) the identity behind the kernels' structure ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BASES))
def test_drop_of_acc_plus_p_z_is_drop_of_acc_plus_z(name):
    """modswitch_oracle.crafted_tile: every prescribed remainder of the drop and every final residue 0, 1, q - 2, q - 1.  Adding
    [p]_(q_r) z_r to the kept residues and nothing to the special prime's shifts the dropped value by exactly z_r modulo q_r, for z = 0, 1,
    q_r - 1 and random z -- also where the sum wraps past q_r"""
    q, n = BASES[name], 256
    L, p = len(q) - 1, q[-1]
    tile = mo.crafted_tile(q, L, n)
    base = mo.switch_residues_levels(tile, q)[L]
    rng = np.random.default_rng(len(name))
    for kind in ("zero", "one", "top", "random"):
        z = [{"zero": np.zeros(n, dtype=object), "one": np.ones(n, dtype=object), "top": np.full(n, qr - 1, dtype=object),
              "random": rs._obj(rng.integers(0, qr, size=n, dtype=np.uint64))}[kind] for qr in q[:L]]
        moved = tile.copy()
        for r in range(L):
            moved[r] = rs._u64((rs._obj(tile[r]) + (p % q[r]) * z[r]) % q[r])
        got = mo.switch_residues_levels(moved, q)[L]
        for r in range(L):
            assert np.array_equal(rs._obj(got[r]), (rs._obj(base[r]) + z[r]) % q[r]), (name, kind, r)
        # one coefficient at a time through the kernel's own arithmetic (the Shoup product of the drop)
        for x in range(0, n, 17):
            assert mo.switch_model([int(moved[i][x]) for i in range(L + 1)], q, L) == [int(v[x]) for v in got]


# ---- (c) decryption and noise on a toy BFV -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("Q3", 32), ("Q4", 32), ("Q4", 64)])
def test_toy_bfv_decrypts_slot_by_slot_within_the_noise_bound(fhe, name, n):
    """one encryption through the fused definition in big integers: every slot is sum_j d_j (.) rot_j(m) modulo t, the EXACT budget is at
    or above rotate_diag_budget of the exact budget before; the op-by-op composition (rotate, multiply_plain, add) decrypts to the same"""
    t = T
    B = fhe.package.keys._Sampler.NOISE_MAX
    q = BASES[name]
    ctx = SimpleNamespace(n=n, t=t, q=q, k=len(q))
    Q = mo.prod(q[:-1])
    rng = np.random.default_rng(n + len(name))
    s = [int(v) - 1 for v in rng.integers(0, 3, size=n)]
    slots = [int(v) for v in rng.integers(0, t, size=n)]
    m = [int(v) for v in go.encode_slots(slots, n, t)]
    a = tk._encrypt(rng, m, s, Q, t)
    worst, plain = tk._worst(a, s, Q, t)
    assert plain == m
    fresh = tk._exact_budget(Q, worst)
    moves = {g: (left, swap) for g, left, swap in go.elements(n)}
    moves[1] = (0, False)
    elts = tr._taps5(n)
    diags = [[int(v) for v in rng.integers(0, 2, size=n)] for _ in elts]       # 0/1 masks ...
    diags[1] = [int(v) for v in rng.integers(0, 4, size=n)]                    # ... and small weights
    plains = [[int(v) for v in go.encode_slots(d, n, t)] for d in diags]
    K = []
    for g in elts:
        sg = s if g == 1 else [tk._centre(v, 3) for v in ks.sigma_big([v % 3 for v in s], g, 3)]
        K.append(None if g == 1 else tk._toy_key(rng, q, s, sg, B))
    want = np.zeros(n, dtype=object)
    for g, d in zip(elts, diags):
        want = (want + np.array(d, dtype=object) * go.permute_slots(np.array(slots, dtype=object), *moves[g])) % t
    fused = rd.rotate_diag_sum_composed(q, t, a, elts, plains, K)
    worst, plain = tk._worst(fused, s, Q, t)
    assert tr._slots_of(plain, n, t) == [int(v) for v in want]
    after = tk._exact_budget(Q, worst)
    bound = fhe.circuits.rotate_diag_budget(ctx, fresh, plains)
    acc = [[0] * n, [0] * n]
    for g, pj, Kj in zip(elts, plains, K):
        if g == 1:
            rot = a
        else:
            sig = [ks.sigma_big(p, g, Q) for p in a]
            u = ks.key_switch_composed(q, [[v % qi for v in sig[1]] for qi in q[:-1]], Kj)
            rot = [[(x + y) % Q for x, y in zip(sig[0], u[0])], u[1]]
        pc = [v % Q for v in rd.centred_poly(pj, t)]
        acc = [[(x + y) % Q for x, y in zip(acc[pp], mo.negacyclic_mul(pc, rot[pp], Q))] for pp in range(2)]
    worst_op, plain_op = tk._worst(acc, s, Q, t)
    assert plain_op == plain, "the fused sum and the op-by-op composition decrypt to the same plaintext"
    W = sum(sum(abs(v) for v in rd.centred_poly(p, t)) for p in plains)
    print("\n[toy BFV rotate_diag_sum %s n=%d taps=%d W=%d] fresh %.1f bits -> fused %.1f, op-by-op %.1f (bound %.1f)"
          % (name, n, len(elts), W, fresh, after, tk._exact_budget(Q, worst_op), bound))
    assert after >= bound - 1e-9


def test_budget_formula(fhe):
    import math
    from fractions import Fraction
    c = fhe.circuits
    B19 = fhe.package.keys._Sampler.NOISE_MAX
    q, n, t = BASES["Q4"], 8192, 65537
    ctx = SimpleNamespace(n=n, t=t, q=q)
    p, Q = q[-1], mo.prod(q[:-1])
    plains = np.zeros((2, n), dtype=np.uint64)
    plains[0, :3] = [1, t - 1, (t + 1) // 2]
    plains[1, n - 1] = 5
    W = 1 + 1 + (t - 1) // 2 + 5
    E = Fraction(W * n * B19 * sum(qi - 1 for qi in q[:-1]), p) + Fraction(1 + n, 2)
    for budget in (40, 77.5):
        want = -math.log2(W * Fraction(2.0 ** -budget) + 2 * t * E / Q)
        assert c.rotate_diag_budget(ctx, budget, plains) == pytest.approx(want, abs=1e-6)
        consts = np.zeros((3, n), dtype=np.uint64)
        consts[:, 0] = [1, t - 2, 7]
        assert c.rotate_diag_budget(ctx, budget, consts) == pytest.approx(c.rotate_sum_budget(ctx, budget, [1, t - 2, 7]), abs=1e-9)
    with pytest.raises(ValueError):
        c.rotate_diag_budget(ctx, 50, np.zeros((1, n), dtype=np.uint64))
    with pytest.raises(ValueError):
        c.rotate_diag_budget(SimpleNamespace(n=n, t=t, q=q[:1]), 50, plains)


# ---- (d) wrong variants, in the model only -------------------------------------------------------------------------------------------------
def test_wrong_variants_are_caught(oracle_mod):
    """(changed crafted outputs, crafted outputs, changed random outputs, random outputs) per variant, Q4 at n = 64, taps {1, 3, 2n - 1,
    3^(n/8), 3^-1}, plaintexts with the edge coefficients and (t - 1) X^(n-1).  Crafted: c_0 and c_1 of family R.
         diag_first  the diagonal applied before the rotation (rotate(multiply_plain(ct, p)))
         perm_inv    pi_(g^-1) used for pi_g
         uncentred   the lift taken uncentred
         c0_special  the c_0 term also added at the special prime
         no_id_c1    the identity tap's p' c_1 left out
    Counts of this run: diag_first, perm_inv and uncentred change 384 of 384 crafted and 384 of 384 random outputs; c0_special 192 of 384
    each (the whole first polynomial); no_id_c1 192 of 384 each (the whole second polynomial)."""
    name, n = "Q4", N_SMALL
    q = BASES[name]
    elts = tr._taps5(n)
    orc, rand, _, ko = tr._setup(oracle_mod, name, elts, seed=11)
    plains = _plains(n, len(elts), seed=2)
    crafted = np.stack([ks.reduction_poly(q, n, 3), ks.reduction_poly(q, n, 2 * n - 1)])
    report = {}
    for variant in rd.VARIANTS:
        row = []
        for ct in (crafted, rand):
            good = rd.rotate_diag_sum(orc, ct, T, elts, plains, ko)
            bad = rd.rotate_diag_sum(orc, ct, T, elts, plains, ko, variant=variant)
            row += [int((good != bad).sum()), good.size]
        report[variant] = tuple(row)
    print("\n[rotate_diag_sum: wrong variants] variant: (crafted changed, crafted, random changed, random) = %r" % report)
    for variant, (cb, ca, rb, ra) in report.items():
        assert cb > 0, variant
        assert rb > 0, variant
    # with constant plaintexts a permuted diagonal is the same diagonal: diag_first changes nothing
    consts = [rd.constant(n, w) for w in rs.edge_weights(T) + [T - 7]]
    assert np.array_equal(rd.rotate_diag_sum(orc, rand, T, elts, consts, ko), rd.rotate_diag_sum(orc, rand, T, elts, consts, ko, variant="diag_first"))


# ---- (e) the host helpers against plain numpy ------------------------------------------------------------------------------------------------
def _apply_diagonals(n, elts, diags, slots, t):
    """sum_j d_j (.) rot_j(slots) on flat slots, from the elements' steps: element 3^s mod 2n rotates both rows LEFT by s"""
    half = n // 2
    step_of = {pow(3, s, 2 * n): s for s in range(half)}
    rows = np.asarray(slots, dtype=object).reshape(2, half)
    out = np.zeros((2, half), dtype=object)
    for g, d in zip(elts, diags):
        out = (out + np.asarray(d, dtype=object).reshape(2, half) * np.roll(rows, -step_of[g], axis=1)) % t
    return out.reshape(n)


@pytest.mark.parametrize("border", ["zero", "clamp"])
@pytest.mark.parametrize("kw,kh,tile_w,anchor", [(3, 3, 8, None), (3, 3, 32, None), (5, 5, 8, None), (5, 5, 32, None), (3, 3, 8, (0, 0)), (5, 5, 32, (4, 4)), (3, 2, 8, (2, 0))])
def test_packed_filter_diagonals_against_numpy(fhe, kw, kh, tile_w, anchor, border):
    c = fhe.circuits
    n, t = 1024, T
    half = n // 2
    tile_h = half // tile_w
    rng = np.random.default_rng(kw * 100 + tile_w)
    w = [int(v) for v in rng.integers(1, 50, size=kw * kh)]
    w[1] = t - 3                                                        # a negative weight
    w[kw] = 0                                                           # and a zero one
    elts, diags = c.packed_filter_diagonals(n, t, tile_w, w, kw, kh, anchor, border)
    assert len(set(elts)) == len(elts) and diags.shape == (len(elts), n) and all(d.any() for d in diags)
    kernel_elts = set(fhe.galois_element(n, (j - (anchor or c.filter_anchor(kw, kh))[1]) * tile_w + (i - (anchor or c.filter_anchor(kw, kh))[0]))
                      for j in range(kh) for i in range(kw))
    assert set(elts) <= kernel_elts, "a border needs no rotation outside the kernel's own"
    tiles = rng.integers(0, 256, size=(2, tile_h, tile_w))
    got = _apply_diagonals(n, elts, diags, tiles.reshape(n), t).reshape(2, tile_h, tile_w)
    for row in range(2):
        want = c.packed_filter_border_model(tiles[row], w, kw, kh, t, anchor, border)
        assert np.array_equal(got[row], want), (border, np.argwhere(got[row] != want)[:4])
    # the model itself against numpy's padding
    ax, ay = anchor or c.filter_anchor(kw, kh)
    pad = np.pad(tiles[0], ((ay, kh - 1 - ay), (ax, kw - 1 - ax)), mode="constant" if border == "zero" else "edge").astype(object)
    direct = sum(int(w[j * kw + i]) * pad[j:j + tile_h, i:i + tile_w] for j in range(kh) for i in range(kw)) % t
    assert np.array_equal(direct, c.packed_filter_border_model(tiles[0], w, kw, kh, t, anchor, border))
    if border == "zero":                                               # inside the valid mask the diagonals are the plain weights
        ok = c.packed_filter_valid_mask(n, tile_w, kw, kh, anchor)
        e0, w0 = c.packed_filter_taps(n, t, tile_w, w, kw, kh, anchor)
        for g, wp in zip(e0, w0):
            assert set(diags[elts.index(g)][ok].tolist()) == {wp}


def test_packed_filter_diagonals_refusals(fhe):
    c = fhe.circuits
    with pytest.raises(ValueError, match="border"):
        c.packed_filter_diagonals(1024, T, 32, [1] * 9, 3, 3, border="wrap")
    with pytest.raises(ValueError, match="weights for"):
        c.packed_filter_diagonals(1024, T, 32, [1] * 8, 3, 3)
    with pytest.raises(ValueError, match="tile_w"):
        c.packed_filter_diagonals(1024, T, 24, [1] * 9, 3, 3)
    with pytest.raises(ValueError, match="anchor inside"):
        c.packed_filter_diagonals(1024, T, 32, [1] * 9, 3, 3, anchor=(3, 0), border="clamp")
    with pytest.raises(ValueError, match="every weight is zero"):
        c.packed_filter_diagonals(1024, T, 32, [0, T] + [0] * 7, 3, 3)


@pytest.mark.parametrize("d", [2, 8])
def test_block_matvec_diagonals_against_numpy(fhe, d):
    c = fhe.circuits
    n, t = 1024, T
    rng = np.random.default_rng(d)
    B = rng.integers(-300, 300, size=(d, d))
    elts, diags = c.block_matvec_diagonals(n, t, B)
    assert elts == [fhe.galois_element(n, s) for s in range(-(d - 1), d)] and diags.shape == (2 * d - 1, n)
    x = rng.integers(0, t, size=n)
    got = _apply_diagonals(n, elts, diags, x, t)
    want = (np.einsum("ab,gb->ga", B.astype(object), x.reshape(n // d, d).astype(object)) % t).reshape(n)
    assert np.array_equal(got, want)
    lower = np.tril(np.ones((d, d), dtype=np.int64))                    # all-zero diagonals are left out
    elts, diags = c.block_matvec_diagonals(n, t, lower)
    assert elts == [fhe.galois_element(n, s) for s in range(-(d - 1), 1)]
    with pytest.raises(ValueError, match="does not divide"):
        c.block_matvec_diagonals(n, t, np.ones((3, 3)))
    with pytest.raises(ValueError, match="square"):
        c.block_matvec_diagonals(n, t, np.ones((2, 3)))
    with pytest.raises(ValueError, match="zero modulo t"):
        c.block_matvec_diagonals(n, t, np.zeros((2, 2)))


# ---- (f) refusals that need no device, and the library's entry points ---------------------------------------------------------------------------
def test_host_side_refusals(fhe):
    n, t = 1024, T
    level = SimpleNamespace(n=n, t=t, k=3, q=BASES["Q4"][:3], device="cpu")
    parent = SimpleNamespace(n=n, t=t, k=4, q=BASES["Q4"], device="cpu", h=None)
    keys = fhe.SpecialGaloisKeys(parent, {})
    ones = lambda G: np.ones((G, n), dtype=np.uint64)
    mk = lambda e, d=None, k=keys, **kw: fhe.RotDiagPlan(level, k, e, ones(len(e)) if d is None else d, **kw)
    for bad, what in (([], "taps"), (list(range(1, 131, 2)), "taps"), ([4], "odd"), ([2 * n + 1], "odd"), ([0], "odd"), ([3, 5, 3], "repeated")):
        with pytest.raises(ValueError, match=what):
            mk(bad)
    with pytest.raises(ValueError, match="diagonals of shape"):
        mk([1, 3], ones(1))
    with pytest.raises(ValueError, match="0 modulo t in every slot"):
        mk([1, 3], np.stack([np.ones(n, dtype=np.uint64), np.full(n, t, dtype=np.uint64)]))
    with pytest.raises(ValueError, match="no special Galois key for element 3"):
        mk([1, 3])
    with pytest.raises(ValueError, match="SpecialGaloisKeys expected"):
        mk([1], k=fhe.GaloisKeys(parent, 30, {}))
    good = [rd.constant(n, 1), rd.constant(n, 2)]
    for elts, plains, why in (([1, 3], good, None), ([], [], "tap count"), ([3, 3], good, "repeated"), ([2], good[:1], "odd"),
                              ([3], [np.zeros(n, dtype=np.uint64)], "zero polynomial"), ([3], [rd.constant(n, t)], "not below t"),
                              ([1, 3], good[:1], "one plaintext per tap")):
        got = rd.check_taps(n, t, 2, elts, plains)
        assert (got is None) if why is None else (why in got)
    assert rd.check_taps(n, t, 1, [3], good[:1]) is not None


def test_library_exports_the_entry_points(fhe):
    lib = fhe._lib.load()
    header = open(fhe.HEADER_PATH).read()
    for name in ("fhe_rotdiag_plan_create", "fhe_rotdiag_plan_destroy", "fhe_rotdiag_scratch_bytes", "fhe_rotate_diag_sum_sp"):
        assert hasattr(lib, name) and name in fhe._lib.SIGNATURES and name in header, name
    assert lib.fhe_rotdiag_scratch_bytes(None, 3) == 0 and lib.fhe_rotdiag_plan_destroy(None) == 0
    assert lib.fhe_rotdiag_plan_create(None, 1, None, None, None, None) == -1
    assert lib.fhe_rotate_diag_sum_sp(None, None, 0, None, 0, 1, None, 0, None) == -1
    assert lib.fhe_abi_version() == 4


# ---- (g) the plan's host code under the host sanitizers -------------------------------------------------------------------------------------
def test_plan_host_code_under_address_and_undefined_sanitizers(tmp_path):
    """tools/rotdiag_host_check.cpp: a program of its own around csrc/rotdiag_host.h (no device, nothing loaded into Python), built with
    -fsanitize=address,undefined and run once"""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rotdiag_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "rotdiag_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout[-2000:], out.stderr[-2000:])
