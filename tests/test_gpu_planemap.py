"""GPU: sparse integer maps across position-packed ciphertexts (include/fhe_hip.h fhe_plane_map; csrc/planemap.hip) against the
specification (tests/planemap_oracle.py, whose two forms tests/test_planemap_cpu.py checks against each other on the unchanged oracle):
bit-exact at the chunk edges of the arithmetic on random residues and on residues q_i - 1, every window and the direct kernel, fused ==
op-by-op through the Evaluator, the cut into groups, packed resize / tile filter / tile resize end to end on real encryptions, refusals,
and the C++ host."""
import ctypes as C
import os

import numpy as np
import pytest

import galois_oracle as go
import packed_oracle as po
import planemap_oracle as pmo
from test_gpu_galois import BASES, _primes_58, _unreduced
from test_gpu_packed import _prime_61

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boazbarak_stb_rgb.npy")
_cache = {}


def _ctx(fhe, name, t=po.T33, direct=False):
    """(context, Evaluator); direct: a context created with FHE_PLANEMAP_DIRECT=1 (the baseline kernel)"""
    if (name, t, direct) not in _cache:
        if name == "Q61":
            n, q, sw = 1024, [_prime_61(1024), go.Q4[0]], {}
        else:
            n, q, sw = BASES[name]
            q = _primes_58(n, 2) if q is None else q
        sw = dict(sw, FHE_PLANEMAP_DIRECT="1") if direct else sw
        ctx = fhe.SEALContext(n, q, t, switches=sw or None)
        _cache[(name, t, direct)] = (ctx, fhe.Evaluator(ctx))
    return _cache[(name, t, direct)]


def _top(fhe, ctx, planes, size):
    return fhe.to_device(np.broadcast_to(np.array(ctx.q, dtype=np.uint64)[None, None, None, :, None] - np.uint64(1), (2, planes, size, ctx.k, ctx.n)).copy(), ctx.device)


@pytest.mark.parametrize("name,size", [(b, s) for b in ("Q3", "Q4", "Q58", "shoup", "Q61") for s in (2, 3)])
def test_plane_map_matches_the_specification(fhe, name, size):
    """n_in = 70, n_out = 41, T = 64, count 2: outputs of exactly 1, 8, 9, 16, 17 and 64 live terms among random ones, zeros, repeated
    sources, +-limit weights, a shuffled order; windows 16, 32, 64 and the direct kernel"""
    import torch
    ctx, ev = _ctx(fhe, name)
    dctx, dev = _ctx(fhe, name, direct=True)
    n_in, n_out, T = 70, 41, 64
    rng = np.random.default_rng(size * 100 + len(name))
    taps, w, order = pmo.random_plan(rng, ctx.t, n_in, n_out, T, pmo.EDGE_TERMS)
    assert sorted(set((w != 0).sum(axis=1)) & set(pmo.EDGE_TERMS)) == list(pmo.EDGE_TERMS)
    print("\n[plane_map %s n=%d k=%d size=%d] arith path %d, max prime %d bits" % (name, ctx.n, ctx.k, size, fhe._lib.load().fhe_arith_path(ctx.h), max(q.bit_length() for q in ctx.q)))
    ct = ctx.random_ct(2, n_in, size=size, seed=fhe.SEED + size)
    top = _top(fhe, ctx, n_in, size)
    plans = [(ev, fhe.PlaneMapPlan(ctx, n_in, taps, w, order=order, window=win)) for win in (16, 32, 64)]
    plans.append((dev, fhe.PlaneMapPlan(dctx, n_in, taps, w, order=order)))
    plans.append((ev, fhe.PlaneMapPlan(ctx, n_in, taps, w, order=order)))                 # window 0: the library's default kernel and cut
    assert [p.window for _, p in plans[:3]] == [16, 32, 64] and plans[0][1].groups >= plans[1][1].groups >= plans[2][1].groups >= 1
    for batch in (ct, top):
        host = fhe.to_host(batch)
        if batch is top:                                               # every coefficient alike: the specification of one, repeated
            want = np.broadcast_to(pmo.plane_map_direct(ctx.q, host[..., :1], taps, w), host.shape[:1] + (n_out,) + host.shape[2:])
        else:
            want = pmo.plane_map_direct(ctx.q, host, taps, w)
        outs = []
        for e, plan in plans:
            out = e.plane_map(plan, batch)
            assert tuple(out.shape) == (batch.shape[0], n_out, size, ctx.k, ctx.n)
            assert np.array_equal(fhe.to_host(out), want), (name, size, plan.window, e is dev)
            assert _unreduced(fhe, e.ctx, out) == 0
            assert torch.equal(batch, fhe.to_device(host, ctx.device)), "the input was written"
            outs.append(out)
        assert torch.equal(outs[2], outs[3]), "window 64 and the direct kernel differ"


@pytest.mark.parametrize("name", ["P4096", "P8192"])
def test_resize_pass_at_the_presets(fhe, name):
    """the horizontal pass of 16x16 -> 8x8 (Catmull-Rom, 8 bits) on one frame at the presets' sizes: the default kernel and the windowed
    one with windows 16 and 64 (the workgroup-to-prime index at n = 4096 / 8192 and the presets' k)"""
    import torch
    ctx, ev = _ctx(fhe, name)
    ct = ctx.random_ct(1, 256, seed=fhe.SEED + 3)
    want = None
    for window in (0, 16, 64):
        h, _ = fhe.circuits.packed_resize_plans(ctx, 16, 16, 8, 8, window=window)
        out = ev.plane_map(h.plan, ct)
        if want is None:
            want = out
            assert np.array_equal(fhe.to_host(out), pmo.plane_map_direct(ctx.q, fhe.to_host(ct), h.taps, h.weights))
        assert torch.equal(out, want), window
        assert _unreduced(fhe, ctx, out) == 0


def test_groups_and_source_reads(fhe):
    import torch
    ctx, ev = _ctx(fhe, "Q3")
    circuits = fhe.circuits
    h64, v64 = circuits.packed_resize_plans(ctx, 16, 16, 8, 8, window=64)
    assert h64.plan.window == 64 and h64.plan.source_reads == 256 and h64.plan.groups == 4          # four rows of 16 sources per group: each source once
    assert v64.plan.source_reads == 128 and v64.plan.groups == 2                                      # columns of 16 sources: four per group
    h16, v16 = circuits.packed_resize_plans(ctx, 16, 16, 8, 8, window=16)
    assert h16.plan.groups == 16 > h64.plan.groups and h16.plan.source_reads == 256 and v16.plan.groups == 8
    v_rows = fhe.PlaneMapPlan(ctx, v64.n_in, v64.taps, v64.weights, window=16)                       # index order: a group holds pieces of many columns
    assert v_rows.source_reads > v16.plan.source_reads
    default = circuits.packed_resize_plans(ctx, 16, 16, 8, 8)[0].plan
    assert default.window in (16, 32, 64)
    ct = ctx.random_ct(2, 256)
    a = circuits.packed_resize(ev, (h64, v64), ct)
    assert torch.equal(a, circuits.packed_resize(ev, (h16, v16), ct)) and torch.equal(a, ev.plane_map(v_rows, ev.plane_map(default, ct)))
    # an output of 64 distinct live sources under window 16 gets a group of its own and still runs
    taps = np.vstack([np.arange(64), np.arange(64) % 5 + 64, np.arange(64)[::-1] + 3]).astype(np.uint32)
    w = np.ones((3, 64), dtype=np.int64)
    w[1, 5:] = 0
    wide = fhe.PlaneMapPlan(ctx, 70, taps, w, window=16)
    assert wide.window == 16 and wide.groups == 3 and wide.source_reads == 64 + 5 + 64
    ct = ctx.random_ct(1, 70)
    assert np.array_equal(fhe.to_host(ev.plane_map(wide, ct)), pmo.plane_map_direct(ctx.q, fhe.to_host(ct), taps, w))


@pytest.mark.parametrize("name", ["Q3", "Q4"])
def test_fused_equals_op_by_op(fhe, name):
    import torch
    ctx, ev = _ctx(fhe, name)
    rng = np.random.default_rng(8)
    taps, w, order = pmo.random_plan(rng, ctx.t, 12, 7, 18, (1, 9, 17))
    ct = ctx.random_ct(1, 12, seed=fhe.SEED + 2)
    want = []
    for o in range(7):
        acc = None
        for tp, wt in zip(taps[o], w[o]):
            if int(wt):
                term = ev.multiply_plain(ct[0, int(tp)], np.array([int(wt) % ctx.t], dtype=np.uint64))
                acc = term if acc is None else ev.add(acc, term)
        want.append(acc)
    assert torch.equal(ev.plane_map(fhe.PlaneMapPlan(ctx, 12, taps, w, order=order), ct)[0], torch.stack(want))


def _client(fhe):
    if "client" not in _cache:
        ctx = fhe.SEALContext(1024, go.Q4, po.T33)
        kg = fhe.KeyGenerator(ctx, seed=13)
        _cache["client"] = (ctx, fhe.DeviceEncryptor(ctx, kg.public_key(), key=bytes(range(32)), reproducible=True), fhe.Decryptor(ctx, kg.secret_key()),
                            fhe.BatchEncoder(ctx), fhe.Evaluator(ctx))
    return _cache["client"]


def _decrypt(dec, be, ct):
    plain, budget = dec.decrypt_batch(ct, with_budget=True)
    return be.decode(plain), min(budget)


def test_packed_resize_and_filters_end_to_end(fhe):
    """n = 1024, the Q4 primes, t = T33: 1024 frames of 16x16 pixels in 256 ciphertexts (frame 0 the golden image's top-left crop) ->
    packed_resize to 8x8 and a box 3x3 tile filter: the decrypted slots are the integer model modulo t; one tile resize of the whole
    48x48 golden channel (core 16 -> 8), stitched, is the whole-image model"""
    ctx, enc, dec, be, ev = _client(fhe)
    circuits, client = fhe.circuits, fhe.client
    t, n = ctx.t, ctx.n
    green = np.load(GOLDEN).astype(np.int64)[:, :, 1]
    frames = np.random.default_rng(6).integers(0, 256, size=(n, 16, 16))
    frames[0] = green[:16, :16]
    slots = client.pack_frames(frames, n, t=t)                                             # [1][256][n]
    ct = enc.encrypt_plains(be.encode(slots[0]))                                           # [256, 2, k, n]
    _, fresh = _decrypt(dec, be, ct[:4])
    plans = circuits.packed_resize_plans(ctx, 16, 16, 8, 8)
    assert plans[1].bound(plans[0].bound(255)) < t // 2
    got, budget = _decrypt(dec, be, circuits.packed_resize(ev, plans, ct))
    model = plans[1].model(plans[0].model(slots[0]))
    assert np.array_equal(got.astype(object), model % t)
    print("\n[packed_resize 16x16 -> 8x8, n=1024 Q4 t=33 bits] noise budget %d -> %d bits" % (fresh, budget))
    assert budget > 0
    box = circuits.packed_tile_filter_plan(ctx, 16, 16, circuits.packed_filter_integer("box3")["weights"], 3, 3)
    got, budget = _decrypt(dec, be, ev.plane_map(box.plan, ct))
    assert np.array_equal(got.astype(object), box.model(slots[0]) % t)
    print("[packed box 3x3 over 16x16 tiles] noise budget %d -> %d bits" % (fresh, budget))
    assert budget > 0
    # the whole golden channel as nine overlapping tiles in slots 0 .. 8
    th, tv, halo, core_out = circuits.packed_tile_resize_plans(48, 48, 24, 24, 16, 16, ctx=ctx)
    tiles = client.pack_tiles(green, 16, 16, halo, n, t=t)
    got, budget = _decrypt(dec, be, circuits.packed_resize(ev, (th, tv), enc.encrypt_plains(be.encode(tiles[0]))))
    whole = circuits.packed_resize_plans(None, 48, 48, 24, 24)
    want = np.array(whole[1].model(whole[0].model(green.reshape(-1))), dtype=object).reshape(24, 24)
    assert np.array_equal(client.unpack_tiles(got[None].astype(object), 24, 24, *core_out), want % t)
    print("[packed tile resize 48x48 -> 24x24, core 16, halo %r] noise budget %d bits" % (halo, budget))
    assert budget > 0


def test_refusals(fhe):
    """each case of the specification is FHE_ERR_PARAM before anything is enqueued: the output keeps its sentinel"""
    import torch
    ctx, ev = _ctx(fhe, "Q3")
    L = fhe._lib.load()
    lim = po.scalar_limit(ctx.t)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    p = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else C.c_void_p(t.data_ptr()))
    taps0 = np.array([[0, 1, 2], [2, 3, 9]], dtype=np.uint32)
    w0 = np.array([[1, -2, 0], [3, 0, 0]], dtype=np.int64)                                  # the dead slot [1][2] points past n_in: not looked at

    def create(n_in=4, n_out=2, T=3, taps=taps0, w=w0, order=None, window=0, c=ctx.h):
        h = C.c_void_p()
        rc = L.fhe_plane_map_plan_create(c, n_in, n_out, T, vp(taps), vp(w), vp(order), window, None, C.byref(h))
        assert rc == 0 or not h.value
        if h.value:
            L.fhe_plane_map_plan_destroy(h)
        return rc
    assert create() == 0 and create(order=np.array([1, 0], dtype=np.uint32)) == 0 and all(create(window=x) == 0 for x in (16, 32, 64))
    dead = w0.copy(); dead[1] = 0
    assert create(w=dead) == -1 and b"no live term" in L.fhe_last_error()
    far = taps0.copy(); far[0, 1] = 4
    assert create(taps=far) == -1 and b"n_in" in L.fhe_last_error()
    assert create(T=0) == -1 and b"T =" in L.fhe_last_error()
    assert create(T=65, taps=np.zeros((2, 65), dtype=np.uint32), w=np.ones((2, 65), dtype=np.int64)) == -1
    assert create(n_in=0) == -1 and create(n_out=0) == -1 and create(n_in=65537) == -1 and create(n_out=65537) == -1
    assert create(n_in=65536) == 0
    for win in (1, 8, 17, 48, 128):
        assert create(window=win) == -1 and b"window" in L.fhe_last_error(), win
    for bad in ([0, 0], [0, 2], [1, 1]):
        assert create(order=np.array(bad, dtype=np.uint32)) == -1 and b"permutation" in L.fhe_last_error(), bad
    for x in (lim + 1, -lim - 1, 1 << 31, -(1 << 31), 1 << 40):
        big = w0.copy(); big[0, 2] = x
        assert create(w=big) == -1 and b"out of range" in L.fhe_last_error(), x
    small = fhe.SEALContext(1024, go.Q3, 65537)                                             # (t - 1) / 2 = 32768 is the limit there
    edge = w0.copy(); edge[0, 0] = -32768
    assert create(w=edge, c=small.h) == 0
    edge[0, 0] = 32769
    assert create(w=edge, c=small.h) == -1
    assert create(taps=None) == -1 and create(w=None) == -1 and create(c=None) == -1
    assert L.fhe_plane_map_plan_create(ctx.h, 4, 2, 3, vp(taps0), vp(w0), None, 0, None, None) == -1
    assert L.fhe_plane_map_plan_info(None, None, None, None) == -1
    plan = fhe.PlaneMapPlan(ctx, 4, taps0, w0)
    ctw = 2 * ctx.k * ctx.n
    buf = torch.full((2 * 4 + 2 * 2 + 2, 2, ctx.k, ctx.n), -1, dtype=torch.int64, device=ctx.device)
    ct = buf[:8]
    ct.copy_(ctx.random_ct(8))
    out = buf[8:12]
    at = lambda words: C.c_void_p(buf.data_ptr() + 8 * words)

    def run(pl=plan.h, src=ct, dst=out, size=2, count=2, c=ctx.h):
        return L.fhe_plane_map(c, pl, p(src), p(dst), size, count, None)
    assert run(size=1) == -1 and run(size=0) == -1 and run(size=65) == -1 and b"size" in L.fhe_last_error()
    assert run(src=None) == -1 and run(dst=None) == -1 and run(pl=None) == -1 and run(c=None) == -1
    assert run(c=small.h) == -1 and b"another context" in L.fhe_last_error()
    for dst in (ct, at(ctx.n), at(8 * ctw - 1), at(4 * ctw)):                               # the input itself, inside it, its last word
        assert run(dst=dst) == -1 and b"overlaps" in L.fhe_last_error()
    assert run(src=at(4 * ctw + 1), dst=out) == -1                                          # an input that ends inside the output
    assert run(count=1 << 40) == -1
    assert run(count=0) == 0
    torch.cuda.synchronize()
    assert bool((buf[8:] == -1).all()), "a refused call wrote its output"
    assert run() == 0 and run(src=at(0), dst=at(8 * ctw)) == 0                               # adjacent ranges do not overlap
    torch.cuda.synchronize()
    assert bool((buf[12:] == -1).all()) and not bool((out == -1).all())
    with pytest.raises(ValueError, match="another context"):
        ev.plane_map(fhe.PlaneMapPlan(small, 4, taps0, w0), ct.reshape(2, 4, 2, ctx.k, ctx.n))
    with pytest.raises(ValueError, match="`ct`"):
        ev.plane_map(plan, ctx.random_ct(2, 5))
    with pytest.raises(ValueError, match="`out`"):
        ev.plane_map(plan, ctx.random_ct(2, 4), out=ctx.empty(2, 3))
    with pytest.raises(fhe.FheError, match="out of range"):
        fhe.PlaneMapPlan(ctx, 4, taps0, w0 * (lim + 1))


def test_cpp_host_agrees_with_the_python_host(fhe, tmp_path):
    """seal/planemap_check (seal::hip::PlaneMapPlan + plane_map over the facade) on a stream of seeded ciphertexts: the bytes, the cut and
    the digest of Evaluator.plane_map"""
    import subprocess
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "planemap_check")
    assert os.path.exists(exe), "build() makes seal/planemap_check"
    ctx, ev = _ctx(fhe, "Q4")
    rng = np.random.default_rng(12)
    n_in, n_out, T, frames = 23, 11, 20, 2
    taps, w, order = pmo.random_plan(rng, ctx.t, n_in, n_out, T, (1, 9, 17, 20))
    taps[w == 0] = 0                                                                        # the text file carries them as they are
    plan = fhe.PlaneMapPlan(ctx, n_in, taps, w, order=order, window=16)
    ct = ctx.random_ct(frames, n_in, seed=fhe.SEED + 5)
    fplan, fin, fout, fwant = (str(tmp_path / x) for x in ("plan.txt", "in.ct", "out.ct", "want.ct"))
    with open(fplan, "w") as f:
        f.write("%d %d %d %d %d\n" % (n_in, n_out, T, 16, n_out))
        for arr in (taps, w, order):
            f.write(" ".join(str(int(v)) for v in arr.reshape(-1)) + "\n")
    with open(fin, "wb") as f:
        for c in fhe.to_host(ct).reshape(-1, 2, ctx.k, ctx.n):
            fhe.server.write_ciphertext(f, c)
    want = fhe.to_host(ev.plane_map(plan, ct))
    r = subprocess.run([exe, fplan, fin, fout, str(frames), str(ctx.n), str(ctx.t)] + [str(q) for q in ctx.q], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(fwant, "wb") as f:
        for c in want.reshape(-1, 2, ctx.k, ctx.n):
            fhe.server.write_ciphertext(f, c)
    assert open(fout, "rb").read() == open(fwant, "rb").read()
    flat = want.reshape(-1)
    with np.errstate(over="ignore"):
        digest = int((flat * (np.uint64(2) * np.arange(flat.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))
    assert "groups=%d source_reads=%d window=16 digest=%016x" % (plan.groups, plan.source_reads, digest) in r.stdout, r.stdout
