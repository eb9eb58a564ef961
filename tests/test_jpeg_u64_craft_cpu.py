"""What tests/jpeg_u64_craft.py's value models of the integer JPEG kernels prove, on the CPU (no GPU, no library).  Run with -s for the tables
that DESIGN.md section 3.7.1 quotes.

  validation  on every base of the GPU file, both DCT directions and both colour conversions: the model's outputs equal the CPU oracle's
              op-by-op result on every crafted block and on the random one, and no range assertion of the model fires (no 64-bit wrap, no
              negative difference, every mulvv_pm result below 2^b + 2 delta^2, every noted site below its static bound)
  exits       family E: at each canon_pm exit (inverse columns, forward columns, k_rgb_ntt_pm<.., true>) and each prime the subtraction is
              taken at >= 1000 outputs, not taken at >= 1000, and fold_pm returns exactly q at >= 1; the prescribed residues are what the
              oracle returns; the solver leaves out at most slot_craft.MAX_LEFT_OUT of the slots.  The row kernels have no conditional
              subtraction: they store their lazy values, which the model bounds (below 62 q and 24 q)
  ties        family T / Z / C: in the canonical kernels a sum equals exactly q, a difference exactly 0, an addmod meets (q-1, q-1), and
              k_ycc2rgb's g meets submod(0, 0)
  variants    every name of jpeg_u64_craft.VARIANTS changes a model's output on crafted data of at least one base; a difference offset one
              power of two lower either changes the output (or trips a range assertion), or the interval model shows that no admissible
              input can make it matter: slack
  reach       the largest value per lazy site beside its static bound (sixteenths of q), crafted beside random; exit subtractions taken on
              the random block beside the crafted E block.  Nothing is asserted against these figures except "within the static bound"
"""
import numpy as np
import pytest

import dct_u64_craft as dc
import idct_oracle as io
import jpeg_u64_craft as jc
import slot_craft as sc
from test_pm_arithmetic_model import Pm
from test_pm_arithmetic_model import mulvv_pm as mulvv_pm_int

BASES = list(jc.bases())
PM_BASES = [b for b in BASES if jc.bases()[b][3] == "A"]
CAN_BASES = [b for b in BASES if jc.bases()[b][3] != "A"]
_SM, _DCT, _COL = {}, {}, {}
CAUGHT = {}                                                  # variant -> set of "family / base" that caught it (printed by the last test)
SLACK = {}
SHOW = True                                                  # the tables: captured unless pytest runs with -s


def slot_model(oracle_mod, n, q):
    key = (n, tuple(q))
    if key not in _SM:
        _SM[key] = jc.slot_model(oracle_mod, n, q)
    return _SM[key]


def oracle_dct(sm, oracle_mod, direction, block):
    return io.OracleOps(sm.orc).idct_block(block, oracle_mod.YQT) if direction == "inv" else sm.orc.dct_quant(block, oracle_mod.YQT)


def analyse(oracle_mod, base, direction):
    """the crafted batch of one base and direction through its model, compared with the oracle block by block"""
    if (base, direction) in _DCT:
        return _DCT[(base, direction)]
    n, q, _, cls = jc.bases()[base]
    sm = slot_model(oracle_mod, n, q)
    names, blocks, G, ok = jc.craft_batch(sm, direction)
    res = jc.run_dct(direction, blocks, sm, cls)
    got = jc.to_coeffs(sm, res["final"])
    want = np.stack([oracle_dct(sm, oracle_mod, direction, b) for b in blocks])
    for b, nm in enumerate(names):
        assert np.array_equal(got[b], want[b]), "%s %s %s: the model differs from the oracle" % (base, direction, nm)
    out = dict(sm=sm, cls=cls, names=names, blocks=blocks, G=G, ok=ok, res=res, want=want)
    _DCT[(base, direction)] = out
    return out


def colour(oracle_mod, base, n):
    if (base, n) in _COL:
        return _COL[(base, n)]
    _, q, _, cls = jc.bases(n)[base]
    sm = slot_model(oracle_mod, n, q)
    col = jc.Colour(sm)
    pres = jc.prescribed_pixels(n)
    ycc, Pr, Pb = jc.craft_ycc(col, pres)
    rgb, want, ok = jc.craft_rgb(col, pres)
    exp_rgb = io.OracleOps(sm.orc).ycc_to_rgb_block(ycc)
    exp_ycc = np.empty_like(rgb)
    for p in range(64):
        exp_ycc[0, p], exp_ycc[1, p], exp_ycc[2, p] = sm.orc.rgb_to_ycc(rgb[0, p], rgb[1, p], rgb[2, p])
    out = dict(sm=sm, col=col, cls=cls, pres=pres, ycc=ycc, Pr=Pr, Pb=Pb, rgb=rgb, want=want, ok=ok, exp_rgb=exp_rgb, exp_ycc=exp_ycc)
    _COL[(base, n)] = out
    return out


def note(table, variant, where):
    table.setdefault(variant, []).append(where)


# ---- the pieces the models stand on --------------------------------------------------------------------------------------------------------------
def test_widest_delta_primes_are_what_the_search_finds():
    """the recorded primes are the search's result, class A admits them, and the next smaller candidate of each size is not admitted"""
    for bits, q in zip((55, 52), jc.WIDE):
        assert jc.widest_delta_prime(bits) == q and sc.is_prime(q) and q.bit_length() == bits and q % (1 << 14) == 1
        p = q - (1 << 14)
        while not sc.is_prime(p):
            p -= 1 << 14
        assert jc.admits_class_a(q) and not jc.admits_class_a(p)
        assert jc.true_product_bound(q) > max([jc.true_product_bound(p) for p in jc.PRESET3 if p.bit_length() == bits] + [0])      # lazier than SEAL's own
    assert dc.pm_class(jc.WIDE) == 1 and dc.pm_class(jc.PRESET3) == 1 and dc.pm_class(jc.bases()["Q58"][1]) == 2 and dc.pm_class(jc.bases()["Q61"][1]) == 0


def test_array_mulvv_pm_equals_the_scalar_model():
    import random
    rng = random.Random(11)
    for q in jc.PRESET3 + jc.WIDE + jc.bases()["Q58"][1]:
        m = Pm(q)
        top = (1 << (m.b + 1)) - 1
        xs = [0, 1, q - 1, q, q + 1, top, 1 << m.b, (1 << 32) - 1, 1 << 32] + [rng.randrange(top + 1) for _ in range(400)]
        for w in [0, 1, q - 1, q // 2] + [rng.randrange(q) for _ in range(4)]:
            r = jc.mulvv_pm(np.array(xs, dtype=np.uint64), np.uint64(w), m)
            assert [int(v) for v in r] == [mulvv_pm_int(x, w, m) for x in xs]
    with pytest.raises(AssertionError):
        jc.mulvv_pm(np.array([1 << 57], dtype=np.uint64), np.uint64(1), Pm(jc.PRESET3[0]))


def test_slot_model_product_has_a_python_integer_path_above_57_bits(oracle_mod):
    rng = np.random.default_rng(4)
    for base in ("Q58", "Q61"):
        n, q, _, _ = jc.bases()[base]
        sm = slot_model(oracle_mod, n, q)
        a = rng.integers(0, 1 << 62, size=(sm.k, 64), dtype=np.int64).astype(np.uint64) % sm.P
        b = rng.integers(0, 1 << 62, size=(sm.k, 64), dtype=np.int64).astype(np.uint64) % sm.P
        a[:, 0] = b[:, 0] = sm.P[:, 0] - np.uint64(1)
        prod = sm.mul(a, b)
        for i, p in enumerate(q):
            assert [int(x) for x in prod[i]] == [int(x) * int(y) % p for x, y in zip(a[i], b[i])]


@pytest.mark.parametrize("direction", ["inv", "fwd"])
def test_static_bounds_of_the_source_comments_hold_in_the_interval_model(direction):
    """every input of a line anywhere below I q, products below 6 q: no offset is smaller than its subtrahend, no noted site passes the
    bound the source states, the rows' outputs are below the I of the columns (62 q; 24 q -- the header of k_dct_lines_pm is right: the
    largest row output is an odd one, four products, and output 4 with its offset stays below 8 q)"""
    table, mid, rows_top, cols_top = jc.offset_table(direction, 6.0, False)
    I_cols = jc.LINE[direction][2]
    assert max(hi for _, hi in mid) <= I_cols
    assert max(cols_top.values()) <= 256 and max(rows_top.values()) <= 256
    if direction == "fwd":
        assert mid[4][1] == 8.0 and max(mid[i][1] for i in (1, 3, 5, 7)) == 24.0 and mid[0][1] == 8.0
    else:
        assert max(hi for _, hi in mid) == jc.idct_pm_out(6) == 62
    for (tag, site), (off, need) in table.items():
        assert off >= need, (tag, site)


# ---- DCT: validation, exits, ties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["inv", "fwd"])
@pytest.mark.parametrize("base", BASES)
def test_models_equal_the_oracle_on_every_block(oracle_mod, base, direction):
    a = analyse(oracle_mod, base, direction)
    sm, names = a["sm"], a["names"]
    assert len(names) <= 12 and sm.left_out <= sc.MAX_LEFT_OUT * sm.crafted
    e = names.index("E")
    slots = jc.to_slots(sm, a["want"][e]).reshape(8, 8, 2, sm.k, sm.n)
    assert a["ok"].mean() >= 1 - sc.MAX_LEFT_OUT
    assert np.array_equal(np.where(a["ok"], slots, 0), np.where(a["ok"], a["G"], 0)), "the oracle's outputs are not the prescribed residues"
    z = names.index("Z-zero")
    assert not a["want"][z].any() and not a["res"]["final"][z].any()


@pytest.mark.parametrize("direction", ["inv", "fwd"])
@pytest.mark.parametrize("base", PM_BASES)
def test_family_e_takes_and_skips_the_exit_subtraction(oracle_mod, base, direction):
    a = analyse(oracle_mod, base, direction)
    sm, names = a["sm"], a["names"]
    e, rnd = names.index("E"), names.index("random")
    for i, r in a["res"]["pm"].items():
        q = np.uint64(sm.q[i])
        fe, fr = r["folded"][:, :, e], r["folded"][:, :, rnd]
        taken, skipped, exact = int((fe >= q).sum()), int((fe < q).sum()), int((fe == q).sum())
        assert taken >= 1000 and skipped >= 1000 and exact >= 1, (base, direction, i, taken, skipped, exact)
        low = a["G"][:, :, :, i] < np.uint64(jc.delta_of(sm.q[i]))
        if direction == "inv":                               # a residue below delta under an offset folds to q + r: taken by construction
            carries = (r["lazy"][:, :, e] >> np.uint64(sm.q[i].bit_length())) >= 1
            assert ((fe >= q) | ~(low & carries & a["ok"][:, i])).all()
        if SHOW:
            print("\n%s %s prime %d: exit subtraction taken %d / skipped %d / fold == q %d on E; taken %d of %d on the random block"
                  % (base, direction, i, taken, skipped, exact, int((fr >= q).sum()), fr.size), end="")
    # all-zero: an inverse output without offset stays 0, every output with an offset is a multiple of q and comes back as 0
    z = names.index("Z-zero")
    for i, r in a["res"]["pm"].items():
        lz = r["lazy"][:, :, z]
        assert not (lz % np.uint64(sm.q[i])).any() and (lz == 0).any() and (lz > 0).any()
        assert not r["final"][:, :, z].any()


@pytest.mark.parametrize("base", CAN_BASES)
def test_family_t_meets_the_canonical_ties(oracle_mod, base):
    for direction in ("inv", "fwd"):
        ties = analyse(oracle_mod, base, direction)["res"]["ties"]
        assert ties["sum == q"] > 0 and ties["difference == 0"] > 0, (base, direction, dict(ties))
        if direction == "fwd":
            assert ties["(q-1, q-1)"] > 0
        if SHOW:
            print("\n%s %s ties: %s" % (base, direction, dict(ties)), end="")


def test_reach_of_every_lazy_site_stays_inside_its_static_bound(oracle_mod):
    """Reach.note asserts the bound on every call; here the table: static bound / crafted batch / random block alone, sixteenths of q"""
    for base in PM_BASES:
        for direction in ("inv", "fwd"):
            a = analyse(oracle_mod, base, direction)
            rnd = a["names"].index("random")
            alone = jc.run_dct(direction, a["blocks"][rnd:rnd + 1], a["sm"], "A")["reach"]
            if SHOW:
                print("\n%s %s: site, static bound, crafted batch, random block (sixteenths of q)" % (base, direction))
                for site, (bound, top) in sorted(a["res"]["reach"].items()):
                    assert top <= bound and alone[site][1] <= top
                    print("  %-28s %5d %5d %5d" % (site, bound, top, alone[site][1]))


# ---- colour -----------------------------------------------------------------------------------------------------------------------------------------
COLOUR_CASES = [(b, jc.N) for b in BASES] + [(b, 8192) for b in jc.bases(8192)]


@pytest.mark.parametrize("base,n", COLOUR_CASES)
def test_colour_models_equal_the_oracle_and_meet_their_ties(oracle_mod, base, n):
    c = colour(oracle_mod, base, n)
    sm, col, pres = c["sm"], c["col"], c["pres"]
    assert sm.left_out <= sc.MAX_LEFT_OUT * sm.crafted
    got, ties = jc.ycc2rgb_canonical(col, c["ycc"])
    assert np.array_equal(got, c["exp_rgb"])
    assert ties["0 - 0"] >= 8 * 2 * sm.k * sm.n and ties["sum == q"] > 0 and ties["(q-1, q-1)"] > 0
    got, ties2 = jc.rgb2ycc_canonical(col, c["rgb"])
    assert np.array_equal(got, c["exp_ycc"])
    assert ties2["sum == q"] > 0 and ties2["difference == 0"] > ties2["0 - 0"]
    P, J = sm.P[:, 0], col.J
    # ycc -> rgb: R = Y' + (the prescribed product): the last addmod meets exactly q, q - 1, 0 + 0 and (q-1) + (q-1)
    yy = c["ycc"][0, :pres].copy()
    yy[:, 0] = (yy[:, 0] + col.off) % sm.P
    total = yy.astype(object) + c["Pr"][:pres].astype(object)
    for i, p in enumerate(sm.q):
        seen = set(np.unique(total[:, :, i]).tolist())
        assert {0, p, p - 1, 2 * p - 2} <= seen, (base, i)
        assert np.array_equal(c["exp_rgb"][0, :pres, :, i], (total[:, :, i] % p).astype(np.uint64))
        # coefficient J: polynomial 1 holds the same words and comes back without the offset
        words = {0, p - 1, p - col.offv[i], p - col.offv[i] - 1}
        assert pres >= 4 and set(int(x) for x in c["ycc"][0, :pres, 0, i, J]) == words == set(int(x) for x in c["ycc"][0, :pres, 1, i, J])
        zero_chroma = c["exp_rgb"][:, pres:pres + 8, :, i]
        assert np.array_equal(zero_chroma[0, :, 1], c["ycc"][0, pres:pres + 8, 1, i])                  # polynomial 1: Y itself
        assert np.array_equal(zero_chroma[0, :, 0, J], (c["ycc"][0, pres:pres + 8, 0, i, J] + col.off[i, J]) % P[i])
        assert 0 in set(int(x) for x in zero_chroma[0, :, 0, J])                                          # (q - off) + off: exactly q
    # rgb -> ycc: the prescribed outputs; at J the subtraction meets off - off = 0 and 0 - off, the same words in polynomial 1 stay
    want = c["want"]
    for i, p in enumerate(sm.q):
        okc = bool(c["ok"][i].all())
        assert okc, "a slot of the 3 x 3 system was singular: the coefficients are not the prescribed ones"
        assert np.array_equal(c["exp_ycc"][1:, :pres, :, i], want[1:, :, :, i])
        assert np.array_equal(c["exp_ycc"][0, :pres, 1, i], want[0, :, 1, i])
        exp0 = (want[0, :, 0, i].astype(object) - col.off[i].astype(object)) % p
        assert np.array_equal(c["exp_ycc"][0, :pres, 0, i], exp0.astype(np.uint64))
        atJ = set(int(x) for x in c["exp_ycc"][0, :pres, 0, i, J])
        assert {0, p - 1} <= atJ and {0, p - 1} <= set(int(x) for x in want[0, :, 1, i, J])
    if SHOW:
        print("\n%s n=%d ycc->rgb ties %s; rgb->ycc ties %s" % (base, n, dict(ties), dict(ties2)), end="")


def pm_units(c, n):
    """(pixel, polynomial, prime) units the scalar transform model runs: every prime and polynomial of two pixels at n = 1024, of pixel 0 and
    prime 0 at n = 8192 (52 000 Python-integer products per transform there)"""
    if n == jc.N:                                           # pixel pres + 2: the one whose product G 0.331264 is q + r at every slot
        return [(px, s, i) for px in (0, 1, c["pres"] + 2) for s in range(2) for i in range(c["sm"].k)]
    return [(0, s, 0) for s in range(2)]


@pytest.mark.parametrize("base,n", [(b, n) for b, n in COLOUR_CASES if jc.bases(n)[b][3]])
def test_rgb_pseudo_mersenne_path_equals_the_oracle_and_its_exit_is_driven(oracle_mod, base, n):
    c = colour(oracle_mod, base, n)
    sm, col, cls = c["sm"], c["col"], c["cls"]
    reach, counts = dc.Reach(), {}
    for px, s, i in pm_units(c, n):
        r = jc.rgb_pm_unit(col, c["rgb"][:, px, s, i], i, s, cls, reach)
        assert np.array_equal(r["final"], c["exp_ycc"][:, px, s, i]), (base, n, px, s, i)
        q = np.uint64(sm.q[i])
        t = counts.setdefault(i, [0, 0, 0])
        t[0], t[1], t[2] = t[0] + int((r["folded"] >= q).sum()), t[1] + int((r["folded"] < q).sum()), t[2] + int((r["folded"] == q).sum())
    for i, (taken, skipped, exact) in counts.items():
        assert taken >= 1000 and skipped >= 1000 and exact >= 1, (base, n, i, taken, skipped, exact)
    if SHOW:
        print("\n%s n=%d class %s rgb exit taken / skipped / fold == q per prime: %s; reach %s" % (base, n, cls, counts, dict(reach)), end="")


# ---- the wrong variants ------------------------------------------------------------------------------------------------------------------------------
def _differs(fn, ref):
    """a wrong model either trips one of the range assertions or returns other words"""
    try:
        return not np.array_equal(fn(), ref)
    except AssertionError:
        return True


@pytest.mark.parametrize("variant", ["exit_no_csub", "exit_gt"])
def test_exit_variants_are_caught_at_every_canon_pm_exit(oracle_mod, variant):
    for base in PM_BASES:
        for direction in ("inv", "fwd"):
            a = analyse(oracle_mod, base, direction)
            for fam in ("E", "Z-zero", "random"):
                b = a["names"].index(fam)
                wrong = jc.run_dct(direction, a["blocks"][b:b + 1], a["sm"], "A", var={variant: 1})["final"]
                if not np.array_equal(wrong[0], a["res"]["final"][b]):
                    note(CAUGHT, variant, "%s / %s %s" % (fam, base, direction))
                # behind the kernel: what k_ntt_inv_pm's first butterflies make of the stored words (the only way to the API)
                for i in range(a["sm"].k):
                    assert jc.transform_entry_wraps(a["res"]["final"][b][..., i, :], a["sm"], i) == 0
                    wraps = jc.transform_entry_wraps(wrong[0][..., i, :], a["sm"], i)
                    assert (wraps > 0) == (variant == "exit_no_csub" and fam == "E"), (base, direction, fam, i, wraps)
                    if wraps:
                        note(CAUGHT, variant, "E through the inverse transform / %s %s" % (base, direction))
            assert "E / %s %s" % (base, direction) in CAUGHT.get(variant, [])
            assert "random / %s %s" % (base, direction) not in CAUGHT[variant] or variant == "exit_no_csub"
    for base in ("pmA", "Q58", "wide"):
        c = colour(oracle_mod, base, jc.N)
        hit = False
        for px, s, i in pm_units(c, jc.N):
            r = jc.rgb_pm_unit(c["col"], c["rgb"][:, px, s, i], i, s, c["cls"], dc.Reach(), var={variant: 1})
            hit = hit or not np.array_equal(r["final"], c["exp_ycc"][:, px, s, i])
        assert hit
        note(CAUGHT, variant, "C / %s rgb exit" % base)


def test_canonical_comparison_variants_are_caught(oracle_mod):
    for base in CAN_BASES:
        for direction in ("inv", "fwd"):
            a = analyse(oracle_mod, base, direction)
            for variant in ("addmod_gt", "submod_neg0"):
                for fam in ("E", "T-ties", "T-F1", "Z-top", "random"):
                    b = a["names"].index(fam)
                    wrong = jc.run_dct(direction, a["blocks"][b:b + 1], a["sm"], None, var={variant: 1})["final"]
                    if not np.array_equal(wrong[0], a["res"]["final"][b]):
                        note(CAUGHT, variant, "%s / %s %s" % (fam, base, direction))
        got = {v: CAUGHT.get(v, []) for v in ("addmod_gt", "submod_neg0")}
        assert any(w.endswith("%s inv" % base) for w in got["addmod_gt"]) and any(w.endswith("%s inv" % base) for w in got["submod_neg0"])
        assert not any(w.startswith("random") for w in got["addmod_gt"] + got["submod_neg0"])
        # forward: every path from a sum or a difference to the store passes a product, which returns the canonical residue of q as of 0
        for variant in ("addmod_gt", "submod_neg0"):
            if not any(w.endswith("%s fwd" % base) for w in got[variant]):
                note(SLACK, variant, "k_dct_slots / %s: the scale product heals a stored q" % base)
    for base in BASES:
        c = colour(oracle_mod, base, jc.N)
        for variant in ("addmod_gt", "submod_neg0"):
            if _differs(lambda: jc.ycc2rgb_canonical(c["col"], c["ycc"], {variant: 1})[0], c["exp_rgb"]):
                note(CAUGHT, variant, "C / %s ycc->rgb" % base)
            if _differs(lambda: jc.rgb2ycc_canonical(c["col"], c["rgb"], {variant: 1})[0], c["exp_ycc"]):
                note(CAUGHT, variant, "C / %s rgb->ycc" % base)
        assert "C / %s ycc->rgb" % base in CAUGHT["addmod_gt"] and "C / %s rgb->ycc" % base in CAUGHT["submod_neg0"]
        # submod(0, 0) in k_ycc2rgb's g would leave q in a register in front of the inverse transform: counted, not an output
        assert jc.ycc2rgb_canonical(c["col"], c["ycc"], {"submod_neg0": 1})[1]["q in a register"] > 0


@pytest.mark.parametrize("variant", ["offset_on_poly1", "offset_sign"])
def test_offset_variants_are_caught_by_family_c(oracle_mod, variant):
    for base in BASES:
        c = colour(oracle_mod, base, jc.N)
        assert _differs(lambda: jc.ycc2rgb_canonical(c["col"], c["ycc"], {variant: 1})[0], c["exp_rgb"])
        assert _differs(lambda: jc.rgb2ycc_canonical(c["col"], c["rgb"], {variant: 1})[0], c["exp_ycc"])
        note(CAUGHT, variant, "C / %s both conversions" % base)
        if c["cls"]:                                         # the exit of k_rgb_ntt_pm: the sign shows on polynomial 0, the stray offset on polynomial 1
            s = 0 if variant == "offset_sign" else 1
            r = jc.rgb_pm_unit(c["col"], c["rgb"][:, 0, s, 0], 0, s, c["cls"], dc.Reach(), var={variant: 1})
            assert not np.array_equal(r["final"], c["exp_ycc"][:, 0, s, 0])
            note(CAUGHT, variant, "C / %s rgb exit" % base)


def test_every_difference_offset_one_power_of_two_lower_is_caught_or_slack(oracle_mod):
    """per site of the four line kernels and of k_rgb_combine_pm.  Caught: the model with the halved offset wraps on crafted data (its
    output changes or a range assertion fires).  Slack: the interval model -- rows' inputs as they are, column c given the rows' output c,
    products below 2^b + 2 delta^2 as mulvv_pm's own bound states and the array product asserts on every call -- shows that half the
    offset still covers the subtrahend.  A site that is neither fails here."""
    rows = []
    for base in PM_BASES:
        n, q, _, _ = jc.bases()[base]
        pb = max(jc.true_product_bound(p) for p in q)
        for direction in ("inv", "fwd"):
            a = analyse(oracle_mod, base, direction)
            table = jc.offset_table(direction, pb, True)[0]
            static = jc.offset_table(direction, 6.0, False)[0]
            pick = [a["names"].index(nm) for nm in ("E", "random")]
            ref = a["res"]["final"][pick][..., 0, :]
            for tag in jc.TAGS[direction]:
                for site in jc.LINE[direction][3]:
                    off, need = table[(tag, site)]
                    if off < 2:
                        rows.append((base, tag, site, off, static[(tag, site)][1], need, "no lower power of two"))
                        continue
                    var = {"offset_too_small": (tag, site)}
                    caught = _differs(lambda: jc.run_dct(direction, a["blocks"][pick], a["sm"], "A", var=var, primes=[0])["final"][..., 0, :], ref)
                    slack = off / 2 >= need
                    assert caught or slack, "%s %s %s: neither caught nor slack" % (base, tag, site)
                    assert not (caught and slack)
                    note(CAUGHT if caught else SLACK, "offset_too_small", "%s %s / %s" % (tag, site, base))
                    rows.append((base, tag, site, off, static[(tag, site)][1], need, "caught by E + random" if caught else "slack"))
    for base in ("pmA", "Q58", "wide"):
        c = colour(oracle_mod, base, jc.N)
        cls, q = c["cls"], c["sm"].q[0]
        off = 1 << jc.nc.clog(jc.CLASSES[cls]["RQ"])
        caught = False
        for px, s, i in pm_units(c, jc.N):
            try:
                r = jc.rgb_pm_unit(c["col"], c["rgb"][:, px, s, i], i, s, cls, dc.Reach(), var={"offset_too_small": ("rgb combine", "off")})
                caught = caught or r["underflow"]
            except AssertionError:
                caught = True
        slack = off / 2 >= max(jc.true_product_bound(p) for p in c["sm"].q)
        assert caught != slack, (base, caught, slack)
        note(CAUGHT if caught else SLACK, "offset_too_small", "rgb combine off (class %s) / %s" % (cls, base))
        rows.append((base, "rgb combine", "off", off, jc.CLASSES[cls]["RQ"] / 16, max(jc.true_product_bound(p) for p in c["sm"].q), "caught by C" if caught else "slack"))
    if SHOW:
        print("\nbase, pass, site, offset, offset needed under the static bounds, under the structured interval model (units of q), verdict")
        for r in rows:
            print("  %-5s %-11s %-6s %4d %7.2f %7.3f  %s" % r)


def test_every_variant_is_caught_somewhere(oracle_mod):
    """the table of DESIGN.md 3.7.1.  Last in file order; what the cases above did not leave behind in this process (a -k selection) is run here"""
    if set(CAUGHT) != set(jc.VARIANTS):
        for v in ("exit_no_csub", "exit_gt"):
            test_exit_variants_are_caught_at_every_canon_pm_exit(oracle_mod, v)
        test_canonical_comparison_variants_are_caught(oracle_mod)
        for v in ("offset_on_poly1", "offset_sign"):
            test_offset_variants_are_caught_by_family_c(oracle_mod, v)
        test_every_difference_offset_one_power_of_two_lower_is_caught_or_slack(oracle_mod)
    if SHOW:
        for v in jc.VARIANTS:
            print("\n%s\n  caught: %s\n  slack: %s" % (v, "; ".join(sorted(set(CAUGHT.get(v, [])))) or "-", "; ".join(sorted(set(SLACK.get(v, [])))) or "-"), end="")
    assert set(CAUGHT) == set(jc.VARIANTS)
