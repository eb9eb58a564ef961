"""CPU: the specification of fhe_plane_map holds on the unchanged oracle in both of its forms (tests/planemap_oracle.py); the packed
resize / tile plans, their integer model and bound, and the client packing against exact rational arithmetic and numpy."""
import os
from fractions import Fraction

import numpy as np
import pytest

import galois_oracle as go
import packed_oracle as po
import planemap_oracle as pmo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boazbarak_stb_rgb.npy")
KERNELS = ("triangle", "catmull_rom", "reference_cubic", "lanczos3", "box")


@pytest.mark.parametrize("size", [2, 3])
def test_the_two_forms_of_the_specification_agree(oracle_mod, size):
    """op-by-op on the oracle == direct evaluation modulo q_i at n = 64: random plans with zeros, repeated sources and +-limit weights"""
    n, t = 64, po.T33
    for q in (go.Q3, go.Q4):
        orc = oracle_mod.Oracle(n, q, t)
        rng = np.random.default_rng(size + len(q))
        X = orc.random_ct(20, size=size, seed=3 + size)
        X[5] = np.array(q, dtype=np.uint64)[None, :, None] - np.uint64(1)
        for T, counts in ((1, ()), (5, (1, 5)), (18, (8, 9, 16, 17))):
            taps, w, _ = pmo.random_plan(rng, t, 20, 9, T, counts)
            assert (w == 0).any() or T == 1
            assert abs(w).max() == po.scalar_limit(t)
            want = pmo.plane_map_compose(orc, X, taps, w)
            assert np.array_equal(pmo.plane_map_direct(q, X, taps, w), want), (len(q), size, T)


@pytest.mark.parametrize("kernel", KERNELS)
def test_resize_plan_weights_sum_to_the_scale(fhe, kernel):
    for convention in ("half_pixel", "reference"):
        for antialias in (False, True):
            for (sw, sh, dw, dh), bits in (((48, 40, 24, 17), 8), ((16, 16, 8, 8), 8), ((9, 7, 17, 13), 10)):
                h, v = fhe.circuits.packed_resize_plans(None, sw, sh, dw, dh, kernel=kernel, antialias=antialias, convention=convention, weight_bits=bits)
                assert (h.n_in, h.n_out, v.n_in, v.n_out) == (sh * sw, sh * dw, sh * dw, dh * dw)
                assert h.scale_bits == v.scale_bits == bits and h.plan is None
                assert (h.weights.sum(axis=1) == 1 << bits).all() and (v.weights.sum(axis=1) == 1 << bits).all(), (kernel, convention, antialias)
                assert sorted(v.order) == list(range(dh * dw)) and list(v.order[:dh]) == [y * dw for y in range(dh)]      # column-major


def _exact_resize(img, tx, wx, ty, wy):
    """the separable resize in exact rational arithmetic: axis weights as Fractions"""
    fx = [[Fraction(float(w)) for w in row] for row in wx]
    fy = [[Fraction(float(w)) for w in row] for row in wy]
    mid = [[sum(fx[x][p] * int(img[y][tx[x][p]]) for p in range(len(fx[x]))) for x in range(len(fx))] for y in range(img.shape[0])]
    return [[sum(fy[Y][p] * mid[ty[Y][p]][x] for p in range(len(fy[Y]))) for x in range(len(fx))] for Y in range(len(fy))]


def test_resize_model_is_the_exact_rational_resize_and_close_to_float(fhe):
    """48x48 golden channel -> 24x17, Catmull-Rom, 8 bits: the model of both passes is the exact rational evaluation of the rounded
    weights times 2^16; descaled, it differs from the float64 resize with unrounded weights by at most the bound the plan's own weight
    differences give: |pixel| <= 255, so an axis pass moves a value by at most 255 * sum |delta w|, the vertical pass (weights of absolute
    sum A_y, unrounded) carries the horizontal deviation on, and rounding to an integer adds 1/2"""
    circuits, client = fhe.circuits, fhe.client
    img = np.load(GOLDEN).astype(np.int64)[:, :, 1]
    sh, sw = img.shape
    assert (sw, sh) == (48, 48)
    dw, dh, bits = 24, 17, 8
    for antialias in (False, True):
        h, v = circuits.packed_resize_plans(None, sw, sh, dw, dh, antialias=antialias, weight_bits=bits)
        got = v.model(h.model(img.reshape(-1)))
        tx, wx = circuits.resample_axis_plan(sw, dw, antialias=antialias, weight_bits=bits)
        ty, wy = circuits.resample_axis_plan(sh, dh, antialias=antialias, weight_bits=bits)
        exact = _exact_resize(img, tx, wx, ty, wy)
        assert [int(e * (1 << 2 * bits)) for row in exact for e in row] == list(got) and all(e.denominator <= 1 << 2 * bits for row in exact for e in row)
        # float64 with unrounded weights
        _, ux = circuits.resample_axis_plan(sw, dw, antialias=antialias)
        _, uy = circuits.resample_axis_plan(sh, dh, antialias=antialias)
        H = (img[:, tx].astype(np.float64) * ux[None, :, :]).sum(axis=2)                # [sh][dw]
        ref = (H[ty] * uy[:, :, None]).sum(axis=1)                                      # [dh][dw]
        dx, dy = np.abs(wx - ux).sum(axis=1), np.abs(wy - uy).sum(axis=1)               # per output of each axis
        # |H~ - H| <= 255 dx[x]; |V~ H~ - V H| <= sum_p |wy~| |H~ - H| + |wy~ - wy| |H| with |H| <= 255 sum |ux|
        bound = np.abs(wy).sum(axis=1)[:, None] * 255.0 * dx[None, :] + dy[:, None] * 255.0 * np.abs(ux).sum(axis=1)[None, :] + 0.5
        mine = client.descale(np.array(got, dtype=object) % po.T41, 2 * bits, po.T41).reshape(dh, dw)
        dev = np.abs(mine - ref)
        print("\n[packed resize 48x48 -> 24x17 catmull_rom antialias=%d, %d bits] max |descaled - float64| = %.4f (bound %.4f at that output; largest bound %.4f)"
              % (antialias, bits, dev.max(), bound.reshape(-1)[dev.argmax()], bound.max()))
        assert (dev <= bound + 1e-9).all()


def test_bound_is_attained_by_a_sign_pattern(fhe):
    circuits = fhe.circuits
    h, v = circuits.packed_resize_plans(None, 16, 16, 8, 8, kernel="lanczos3", weight_bits=8)
    box = circuits.packed_tile_filter_plan(None, 8, 8, circuits.packed_filter_integer("sobel_x")["weights"], 3, 3)
    for plan in (h, v, box):
        b = plan.bound(255)
        per_out = (np.abs(plan.weights).astype(object) * 255).sum(axis=1)
        o = int(np.argmax(per_out))
        assert b == int(per_out[o])
        x = np.zeros(plan.n_in, dtype=object)
        for tp, w in zip(plan.taps[o], plan.weights[o]):
            if w:
                x[tp] += 255 * (1 if w > 0 else -1)
        # a source used twice with opposite signs cannot attain the sum; then the bound is an upper bound only
        twice_opposite = any(len({np.sign(w) for tp2, w in zip(plan.taps[o], plan.weights[o]) if w and tp2 == tp}) > 1 for tp in plan.taps[o])
        y = plan.model(np.clip(x, -255, 255))
        assert abs(int(y[o])) == b or twice_opposite
        assert max(abs(int(e)) for e in plan.model(np.clip(x, -255, 255))) <= b
        per_plane = np.arange(plan.n_in) % 7
        assert plan.bound(per_plane) == max(sum(abs(int(w)) * int(per_plane[tp]) for tp, w in zip(trow, wrow) if w) for trow, wrow in zip(plan.taps, plan.weights))


def test_tile_filter_plan_is_the_clamped_filter(fhe):
    circuits = fhe.circuits
    rng = np.random.default_rng(2)
    tile = rng.integers(0, 256, size=(7, 10))
    for name in circuits.FILTERS:
        f = circuits.packed_filter_integer(name)
        kh, kw = f["weights"].shape
        assert np.allclose(f["weights"] / f["divisor"], circuits.FILTERS[name]["weights"])
        plan = circuits.packed_tile_filter_plan(None, 10, 7, f["weights"], kw, kh, anchor=f["anchor"], stride=f["stride"])
        sx, sy = f["stride"]
        assert (plan.dst_w, plan.dst_h) == (-(-10 // sx), -(-7 // sy)) and plan.n_out == plan.dst_w * plan.dst_h and plan.scale_bits == 0
        got = plan.model(tile.reshape(-1)).reshape(plan.dst_h, plan.dst_w)
        ax, ay = f["anchor"]
        for Y in range(plan.dst_h):
            for X in range(plan.dst_w):
                want = sum(int(f["weights"][j][i]) * int(tile[min(max(Y * sy + j - ay, 0), 6)][min(max(X * sx + i - ax, 0), 9)]) for j in range(kh) for i in range(kw))
                assert got[Y][X] == want, (name, X, Y)


@pytest.mark.parametrize("dst,kernel,antialias", [(24, "catmull_rom", False), (36, "catmull_rom", False), (24, "lanczos3", True), (36, "triangle", False)])
def test_tile_plans_stitch_to_the_whole_image_model(fhe, dst, kernel, antialias):
    """48 -> 24 and 48 -> 36 with a core of 16: every tile through the two frame plans, stitched, is the whole-image model exactly"""
    circuits, client = fhe.circuits, fhe.client
    img = np.load(GOLDEN).astype(np.int64)[:, :, 0]
    n = 16
    whole_h, whole_v = circuits.packed_resize_plans(None, 48, 48, dst, dst, kernel=kernel, antialias=antialias)
    want = np.array(whole_v.model(whole_h.model(img.reshape(-1))), dtype=object).reshape(dst, dst)
    th, tv, halo, core_out = circuits.packed_tile_resize_plans(48, 48, dst, dst, 16, 16, kernel=kernel, antialias=antialias)
    assert core_out == (dst // 3, dst // 3) and halo[0] >= (0 if kernel == "triangle" else 1) and th.n_in == (16 + 2 * halo[0]) * (16 + 2 * halo[1])
    slots = client.pack_tiles(img, 16, 16, halo, n)
    assert slots.shape == (1, th.n_in, n) and not slots[0, :, 9:].any()
    out = np.array(tv.model(th.model(slots[0])), dtype=object)[None]
    assert np.array_equal(client.unpack_tiles(out, dst, dst, *core_out), want)


def test_tile_plans_refuse_a_core_that_breaks_periodicity(fhe):
    circuits = fhe.circuits
    with pytest.raises(ValueError, match="tile"):
        circuits.packed_tile_resize_plans(48, 48, 36, 36, 6, 6)          # 6 * 36 / 48 is no integer
    with pytest.raises(ValueError, match="tile"):
        circuits.packed_tile_resize_plans(48, 48, 24, 24, 10, 16)        # 10 does not divide 48
    with pytest.raises(ValueError, match="tile"):
        circuits.packed_tile_resize_plans(48, 48, 17, 17, 16, 16)
    circuits.packed_tile_resize_plans(48, 48, 36, 36, 4, 8)


def test_pack_frames_and_tiles_round_trip(fhe):
    client = fhe.client
    rng = np.random.default_rng(4)
    n, t = 8, 65537
    frames = rng.integers(-300, 300, size=(19, 5, 6))
    slots = client.pack_frames(frames, n)
    assert slots.shape == (3, 30, n) and slots.dtype == np.int64
    assert slots[2, 7, 2] == frames[18].reshape(-1)[7] and not slots[2, :, 3:].any()      # slot b of plane p: pixel p of frame b
    assert np.array_equal(client.unpack_frames(slots, 19, (5, 6)), frames)
    mod = client.pack_frames(frames, n, t=t)
    assert mod.dtype == np.uint64 and np.array_equal(mod.astype(np.int64), slots % t)
    img = rng.integers(0, 256, size=(11, 14))
    for halo in (0, 2, (3, 1)):
        hx, hy = (halo, halo) if isinstance(halo, int) else halo
        slots = client.pack_tiles(img, 4, 5, halo, n)
        tiles = client.unpack_frames(slots, 4 * 3, (5 + 2 * hy, 4 + 2 * hx))
        for b in range(12):
            j, i = divmod(b, 4)
            for y in range(5 + 2 * hy):
                for x in range(4 + 2 * hx):
                    assert tiles[b, y, x] == img[min(max(j * 5 - hy + y, 0), 10), min(max(i * 4 - hx + x, 0), 13)]      # the clamped border
        cores = tiles[:, hy:hy + 5, hx:hx + 4].reshape(12, -1)
        assert np.array_equal(client.unpack_tiles(client.pack_frames(cores, n), 14, 11, 4, 5), img)


def test_lazy_sums_fit_64_bits():
    """the range statement of csrc/planemap.hip: 32 q < 2^64 (in fact <= 2^63) for every base of the GPU test that takes the lazy path"""
    from test_gpu_galois import BASES, _primes_58
    for name, (n, q, sw) in BASES.items():
        q = _primes_58(n, 2) if q is None else q
        lazy = max(x.bit_length() for x in q) <= 58 and "FHE_NTT_NOPM" not in sw
        assert lazy == (name != "shoup")
        if lazy:
            assert all(32 * x <= 1 << 63 for x in q)
        assert all(8 * x < 1 << 64 and x < 1 << 61 for x in q)           # the canonical path: eight products below q
