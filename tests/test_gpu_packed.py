"""GPU: integer linear maps across slot-packed ciphertexts (include/fhe_hip.h fhe_block8x8_scalar / fhe_channel_mix; csrc/packed.hip)
against the specification (tests/packed_oracle.py, whose two forms tests/test_packed_cpu.py checks against each other on the unchanged
oracle): bit-exact on random residues and on residues q_i - 1, fused == op-by-op through the Evaluator, in place == out of place, the
identity plan, strided channel mixes, the packed JPEG transform end to end on real encryptions, refusals, and the C++ host."""
import ctypes as C
import os

import numpy as np
import pytest

import galois_oracle as go
import packed_oracle as po
from test_gpu_galois import BASES, _is_prime, _primes_58, _unreduced

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boazbarak_stb_rgb.npy")
_cache = {}


def _prime_61(n):
    """the largest 61-bit prime = 1 (mod 2n): beyond the lazy sums (eight terms below 4 q do not fit 64 bits), the canonical products run"""
    m = (1 << 61) + 1
    while True:
        m -= 2 * n
        if _is_prime(m):
            return m


def _ctx(fhe, name, t=po.T33):
    if (name, t) not in _cache:
        if name == "Q61":
            n, q, sw = 1024, [_prime_61(1024), go.Q4[0]], {}
        else:
            n, q, sw = BASES[name]
            q = _primes_58(n, 2) if q is None else q
        ctx = fhe.SEALContext(n, q, t, switches=sw or None)
        _cache[(name, t)] = (ctx, fhe.Evaluator(ctx))
    return _cache[(name, t)]


def _plan(fhe, ctx, rng, pre=True, post=True):
    L, R, p0, p1 = po.random_plan(rng, ctx.t, pre, post)
    return fhe.Block8x8Plan(ctx, L, R, p0, p1), (L, R, p0, p1)


@pytest.mark.parametrize("name,count,size", [(b, 2, s) for b in ("Q3", "Q4", "Q58", "shoup", "Q61") for s in (2, 3)] + [("P4096", 1, 2), ("P8192", 1, 2)])
def test_block8x8_matches_the_specification(fhe, name, count, size):
    import torch
    ctx, ev = _ctx(fhe, name)
    rng = np.random.default_rng(size * 100 + len(name))
    print("\n[block8x8 %s n=%d k=%d size=%d] arith path %d, max prime %d bits" % (name, ctx.n, ctx.k, size, fhe._lib.load().fhe_arith_path(ctx.h), max(q.bit_length() for q in ctx.q)))
    ct = ctx.random_ct(count, 64, size=size, seed=fhe.SEED + size)
    top = fhe.to_device(np.broadcast_to(np.array(ctx.q, dtype=np.uint64)[None, None, None, :, None] - np.uint64(1), (1, 64, size, ctx.k, ctx.n)).copy(), ctx.device)
    for pre, post in ((True, True), (False, False)) if ctx.n == 1024 else ((True, True),):
        plan, spec = _plan(fhe, ctx, rng, pre, post)
        for batch in (ct, top):
            host = fhe.to_host(batch)
            out = ev.block8x8_scalar(plan, batch)
            if batch is top:                                           # every coefficient alike: the specification of one, repeated
                want = np.broadcast_to(po.block8x8_direct(ctx.q, host[..., :1], *spec), host.shape)
            else:
                want = po.block8x8_direct(ctx.q, host, *spec)
            assert np.array_equal(fhe.to_host(out), want), (name, size, pre, post)
            assert _unreduced(fhe, ctx, out) == 0
            assert torch.equal(batch, fhe.to_device(host, ctx.device)), "the input was written"
            buf = batch.clone()
            assert ev.block8x8_scalar(plan, buf, out=buf) is buf and torch.equal(buf, out), "in place differs"


def _compose(ev, X, L, R, pre, post):
    """the specification through Evaluator.multiply_plain / add on a device batch X [64, size, k, n]"""
    t = ev.ctx.t

    def scal(a, w):
        return ev.multiply_plain(a, np.array([int(w) % t], dtype=np.uint64))

    def wsum(terms):
        acc = None
        for w, a in terms:
            if int(w):
                term = scal(a, w)
                acc = term if acc is None else ev.add(acc, term)
        return acc
    x = [[X[8 * i + j] if pre is None else scal(X[8 * i + j], pre[i][j]) for j in range(8)] for i in range(8)]
    cols = [[wsum([(L[u][i], x[i][y]) for i in range(8)]) for y in range(8)] for u in range(8)]
    import torch
    return torch.stack([wsum([(R[v][j], cols[u][j]) for j in range(8)]) if post is None else scal(wsum([(R[v][j], cols[u][j]) for j in range(8)]), post[u][v])
                        for u in range(8) for v in range(8)])


@pytest.mark.parametrize("name", ["Q3", "Q4", "shoup"])
def test_fused_equals_op_by_op(fhe, name):
    import torch
    ctx, ev = _ctx(fhe, name)
    rng = np.random.default_rng(5)
    ct = ctx.random_ct(1, 64, seed=fhe.SEED + 1)
    for pre, post in ((True, True), (False, False)):
        plan, spec = _plan(fhe, ctx, rng, pre, post)
        assert torch.equal(ev.block8x8_scalar(plan, ct)[0], _compose(ev, ct[0], *spec)), (name, pre, post)


def test_identity_plan_returns_the_input(fhe):
    import torch
    for name in ("Q3", "Q4", "Q61"):
        ctx, ev = _ctx(fhe, name)
        eye = np.eye(8, dtype=np.int64)
        ct = ctx.random_ct(2, 64, size=3)
        assert torch.equal(ev.block8x8_scalar(fhe.Block8x8Plan(ctx, eye, eye), ct), ct)
        assert torch.equal(ev.block8x8_scalar(fhe.Block8x8Plan(ctx, eye, eye, np.ones((8, 8)), np.ones(64)), ct), ct)
        neg = ev.block8x8_scalar(fhe.Block8x8Plan(ctx, -eye, eye), ct)
        assert torch.equal(neg, ev.negate(ct))
        assert torch.equal(ev.channel_mix(np.eye(3, dtype=np.int64), ct[:, :3].transpose(0, 1).contiguous()), ct[:, :3].transpose(0, 1).contiguous())


@pytest.mark.parametrize("name", ["Q3", "Q4", "Q58", "shoup", "Q61"])
def test_channel_mix(fhe, name):
    """parity at c, m in {1, 3, 8} with and without bias; interleaved and planar strides with sentinel-filled gaps; in place with m == c"""
    import torch
    ctx, ev = _ctx(fhe, name)
    L = fhe._lib.load()
    lim = po.scalar_limit(ctx.t)
    rng = np.random.default_rng(len(name))
    count, size = 3, 2
    ctw = size * ctx.k * ctx.n
    p = lambda t: C.c_void_p(t.data_ptr())
    for c, m in ((1, 1), (3, 3), (8, 8), (3, 1), (1, 8), (8, 3)):
        M = rng.integers(-lim, lim + 1, size=(m, c), dtype=np.int64)
        M[0, 0], M[m - 1, c - 1] = lim, -lim
        if c > 1:
            M[0, 1] = 0
        bias = rng.integers(-lim, lim + 1, size=m, dtype=np.int64)
        bias[0] = -lim
        if m > 1:
            bias[1] = 0
        planes = ctx.random_ct(c, count, size=size, seed=fhe.SEED + c * 8 + m)
        planes[0, 0] = fhe.to_device(np.broadcast_to(np.array(ctx.q, dtype=np.uint64)[None, :, None] - np.uint64(1), (size, ctx.k, ctx.n)).copy(), ctx.device)
        host = fhe.to_host(planes)
        for b in (None, bias):
            want = po.channel_mix_direct(ctx.q, ctx.t, M, host, b)
            out = ev.channel_mix(M, planes, bias=b)
            assert np.array_equal(fhe.to_host(out), want), (name, c, m, b is None)
            assert _unreduced(fhe, ctx, out) == 0 and torch.equal(planes, fhe.to_device(host, ctx.device))
            if m == c:
                buf = planes.clone()
                assert ev.channel_mix(M, buf, bias=b, out=buf) is buf and torch.equal(buf, out), "in place differs"
            # interleaved ([count][channels] with a gap behind every ciphertext) in, planar with gaps out; then the other way round
            gi, go_ = ctw + 2 * ctx.n, ctw + 3 * ctx.n
            src = torch.full((count, c, gi), -1, dtype=torch.int64, device=ctx.device)
            src[:, :, :ctw] = planes.reshape(c, count, ctw).transpose(0, 1)
            dst = torch.full((m, count, go_), -1, dtype=torch.int64, device=ctx.device)
            bp = None if b is None else b.ctypes.data_as(C.c_void_p)
            fhe._lib.call("fhe_channel_mix", ctx.h, M.ctypes.data_as(C.c_void_p), bp, c, m, p(src), c * gi, gi, p(dst), go_, count * go_, size, count, None)
            assert torch.equal(dst[:, :, :ctw].reshape(out.shape), out) and bool((dst[:, :, ctw:] == -1).all()), "interleaved -> planar differs"
            src2 = torch.full((c, count, gi), -1, dtype=torch.int64, device=ctx.device)
            src2[:, :, :ctw] = planes.reshape(c, count, ctw)
            dst2 = torch.full((count, m, go_), -1, dtype=torch.int64, device=ctx.device)
            fhe._lib.call("fhe_channel_mix", ctx.h, M.ctypes.data_as(C.c_void_p), bp, c, m, p(src2), gi, count * gi, p(dst2), m * go_, go_, size, count, None)
            assert torch.equal(dst2[:, :, :ctw].transpose(0, 1).reshape(out.shape), out) and bool((dst2[:, :, ctw:] == -1).all()), "planar -> interleaved differs"
            assert bool((src[:, :, ctw:] == -1).all()) and bool((src2[:, :, ctw:] == -1).all())
    # the op-by-op composition through the Evaluator, 3 x 3 with bias
    M, bias = fhe.circuits.packed_rgb_to_ycc(8), [-(128 << 8), 0, 77]
    planes = ctx.random_ct(3, 2)
    want = []
    for i in range(3):
        acc = None
        for j in range(3):
            term = ev.multiply_plain(planes[j], np.array([int(M[i][j]) % ctx.t], dtype=np.uint64))
            acc = term if acc is None else ev.add(acc, term)
        want.append(ev.add_plain(acc, np.array([bias[i] % ctx.t], dtype=np.uint64)) if bias[i] else acc)
    assert torch.equal(ev.channel_mix(M, planes, bias=bias), torch.stack(want))


def _client(fhe):
    if "client" not in _cache:
        ctx = fhe.SEALContext(8192, go.Q4, po.T41)
        kg = fhe.KeyGenerator(ctx, seed=11)
        _cache["client"] = (ctx, fhe.DeviceEncryptor(ctx, kg.public_key(), key=bytes(range(32)), reproducible=True), fhe.Decryptor(ctx, kg.secret_key()),
                            fhe.BatchEncoder(ctx), fhe.Evaluator(ctx))
    return _cache["client"]


def _encrypt_groups(enc, be, slots):
    """[groups, 64, n] slot values (uint64 below t) -> [groups, 64, 2, k, n]"""
    g = slots.shape[0]
    ct = enc.encrypt_plains(be.encode(slots.reshape(g * 64, -1)))
    return ct.reshape((g, 64) + tuple(ct.shape[1:]))


def _decrypt_groups(dec, be, ct):
    lead = tuple(ct.shape[:-3])
    plain, budget = dec.decrypt_batch(ct.reshape((-1,) + tuple(ct.shape[-3:])), with_budget=True)
    return be.decode(plain).reshape(lead + (-1,)), min(budget)


def test_packed_jpeg_end_to_end(fhe):
    """the golden image at the P8192 primes with the 41-bit batching prime: pack_blocks -> encrypt -> packed_jpeg_compress -> decrypt ->
    unpack_blocks equals the integer model exactly and meets the +-1 / 2 % condition against float64; packed_idct_plan on the descaled,
    re-encrypted coefficients returns the pixels the integer model returns"""
    from test_packed_cpu import check_against_float
    ctx, enc, dec, be, ev = _client(fhe)
    circuits, client = fhe.circuits, fhe.client
    t, n = ctx.t, ctx.n
    rgb = np.load(GOLDEN).astype(np.int64)
    h, w = rgb.shape[:2]
    fwd = circuits.packed_dct_plan(ctx)
    assert fwd.bound(128 << 8) < t // 2
    cts = [_encrypt_groups(enc, be, client.pack_blocks(rgb[:, :, c], w, h, n, t=t)) for c in range(3)]
    _, fresh = _decrypt_groups(dec, be, cts[0])
    out = circuits.packed_jpeg_compress(ev, fwd, *cts)
    assert tuple(out.shape) == (3, 1, 64, 2, ctx.k, n)
    slots, budget = _decrypt_groups(dec, be, out)
    print("\n[packed_jpeg_compress P8192 t=41 bits] noise budget %d -> %d bits" % (fresh, budget))
    assert budget > 0
    # the integer model: colour mix with the level shift, then the block plan, all in Python integers
    M = circuits.packed_rgb_to_ycc(8).astype(object)
    ycc = np.einsum("ij,hwj->ihw", M, rgb.astype(object))
    ycc[0] -= 128 << 8
    Q = np.array(fhe.YQT).reshape(8, 8)
    got, coeffs = [], []
    for c in range(3):
        model = fwd.model(po.blocks8(ycc[c]))                                           # [36, 8, 8]
        mine = po.blocks8(client.unpack_blocks(slots[c], w, h))
        assert np.array_equal(mine.astype(object), model % t), c
        coeffs.append(client.descale(mine, fwd.scale_bits + 8, t))
        got.append(coeffs[-1])
    # against float64 on the exact YCbCr of the pixels (what a JPEG encoder computes), level-shifted
    exact = [0.299 * rgb[:, :, 0] + 0.587 * rgb[:, :, 1] + 0.114 * rgb[:, :, 2] - 128.0,
             -0.168736 * rgb[:, :, 0] - 0.331264 * rgb[:, :, 1] + 0.5 * rgb[:, :, 2],
             0.5 * rgb[:, :, 0] - 0.418688 * rgb[:, :, 1] - 0.081312 * rgb[:, :, 2]]
    check_against_float(got, exact, Q)
    # the way back on one channel: re-encrypt the quantised coefficients, dequantise + inverse DCT, descale
    inv = circuits.packed_idct_plan(ctx)
    assert inv.bound(np.abs(coeffs[0]).max(axis=0)) < t // 2
    nb = len(coeffs[0])                                                                   # 36 blocks: slots 0 .. 35 of one group
    cs = np.zeros((1, 64, n), dtype=np.int64)
    cs[0, :, :nb] = coeffs[0].reshape(nb, 64).T
    back_ct = ev.block8x8_scalar(inv.plan, _encrypt_groups(enc, be, (cs % t).astype(np.uint64)))
    bslots, bbudget = _decrypt_groups(dec, be, back_ct)
    print("[packed idct P8192] noise budget left %d bits" % bbudget)
    assert bbudget > 0
    pixels = client.descale(bslots[0][:, :nb].T.reshape(-1, 8, 8), inv.scale_bits, t)
    model = client.descale(inv.model(coeffs[0]) % t, inv.scale_bits, t)
    assert np.array_equal(pixels, model)
    want = np.floor(exact[0] + 0.5).astype(np.int64)                                      # the bound is the integer model's own error: it is printed, the equality above is the check
    print("[packed idct P8192] max |pixel - original| %d (the model's own error after quantisation)" % int(np.abs(model - po.blocks8(want)).max()))


def test_refusals(fhe):
    """each case of the specification is FHE_ERR_PARAM before anything is enqueued: the output keeps its sentinel"""
    import torch
    ctx, ev = _ctx(fhe, "Q3")
    L = fhe._lib.load()
    lim = po.scalar_limit(ctx.t)
    eye = np.eye(8, dtype=np.int64).reshape(-1)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    p = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else C.c_void_p(t.data_ptr()))

    def create(Lm=eye, Rm=eye, pre=None, post=None, c=ctx.h):
        h = C.c_void_p()
        rc = L.fhe_block8x8_plan_create(c, vp(Lm), vp(Rm), vp(pre), vp(post), None, C.byref(h))
        assert rc == 0 or not h.value
        if h.value:
            L.fhe_block8x8_plan_destroy(h)
        return rc
    ones = np.ones(64, dtype=np.int64)
    assert create() == 0 and create(pre=ones, post=ones) == 0
    bad = ones.copy(); bad[17] = 0
    assert create(pre=bad) == -1 and b"zero" in L.fhe_last_error() and create(post=bad) == -1
    z = eye.copy(); z[8 * 3 + 3] = 0
    assert create(Lm=z) == -1 and b"all zero" in L.fhe_last_error() and create(Rm=z) == -1
    for w in (lim + 1, -lim - 1, 1 << 31, -(1 << 31), 1 << 40):
        big = eye.copy(); big[5] = w
        assert create(Lm=big) == -1 and b"out of range" in L.fhe_last_error(), w
        bigp = ones.copy(); bigp[5] = w
        assert create(Rm=big) == -1 and create(pre=bigp) == -1 and create(post=bigp) == -1
    small = fhe.SEALContext(1024, go.Q3, 65537)                        # (t - 1) / 2 = 32768 is the limit there
    e2 = eye.copy(); e2[0] = 32768
    assert create(Lm=e2, c=small.h) == 0
    e2[0] = 32769
    assert create(Lm=e2, c=small.h) == -1
    assert create(Lm=None) == -1 and create(Rm=None) == -1 and create(c=None) == -1
    plan = fhe.Block8x8Plan(ctx, eye, eye)
    ct = ctx.random_ct(2, 64)
    out = torch.full_like(ct, -1)

    def run(pl=plan.h, src=ct, dst=out, size=2, count=2, c=ctx.h):
        return L.fhe_block8x8_scalar(c, pl, p(src), p(dst), size, count, None)
    assert run(size=1) == -1 and run(size=0) == -1 and run(size=65) == -1 and b"size" in L.fhe_last_error()
    assert run(src=None) == -1 and run(dst=None) == -1 and run(pl=None) == -1 and run(c=None) == -1
    assert run(c=small.h) == -1 and b"another context" in L.fhe_last_error()
    assert run(dst=C.c_void_p(ct.data_ptr() + 8 * ctx.n)) == -1 and b"overlaps" in L.fhe_last_error()
    assert run(count=0) == 0
    M = np.array([[1, 2, 3], [0, 0, 0], [1, 1, 1]], dtype=np.int64)
    planes = ctx.random_ct(3, 2)
    mo = torch.full_like(planes, -1)
    ctw = 2 * ctx.k * ctx.n

    def mix(Mm=np.ones((3, 3), dtype=np.int64), bias=None, c=3, m=3, src=planes, ics=ctw, ips=2 * ctw, dst=mo, ocs=ctw, ops=2 * ctw, size=2, count=2):
        return L.fhe_channel_mix(ctx.h, vp(None if Mm is None else np.ascontiguousarray(Mm)), vp(bias), c, m, p(src), ics, ips, p(dst), ocs, ops, size, count, None)
    assert mix(Mm=M) == -1 and b"all zero" in L.fhe_last_error()
    assert mix(c=0) == -1 and mix(c=9) == -1 and mix(m=0) == -1 and mix(m=9) == -1
    assert mix(Mm=np.full((3, 3), lim + 1, dtype=np.int64)) == -1 and mix(bias=np.array([0, lim + 1, 0], dtype=np.int64)) == -1
    assert mix(size=1) == -1 and mix(src=None) == -1 and mix(dst=None) == -1 and mix(Mm=None) == -1
    assert mix(dst=C.c_void_p(planes.data_ptr() + 8 * ctx.n)) == -1 and b"overlaps" in L.fhe_last_error()
    assert mix(dst=planes, ocs=ctw, ops=2 * ctw, m=2, Mm=np.ones((2, 3), dtype=np.int64)) == -1      # same pointer, m != c
    assert mix(dst=planes, ocs=2 * ctw, ops=ctw, count=1) == -1                                         # same pointer, other strides
    assert mix(ocs=ctw - 1) == -1 and mix(ops=ctw) == -1 and b"strides" in L.fhe_last_error()
    assert mix(ocs=1 << 63, ops=1 << 61) == -1 and b"2^60" in L.fhe_last_error()                      # strides whose extent would wrap 64 bits
    assert run(count=1 << 40) == -1
    assert mix(count=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -1).all()) and bool((mo == -1).all()), "a refused call wrote its output"
    assert mix() == 0
    with pytest.raises(ValueError, match="another context"):
        ev.block8x8_scalar(fhe.Block8x8Plan(small, eye, eye), ct)
    with pytest.raises(ValueError, match="`blocks`"):
        ev.block8x8_scalar(plan, ctx.random_ct(2, 63))
    with pytest.raises(ValueError, match="`out`"):
        ev.block8x8_scalar(plan, ct, out=torch.empty(1, 64, 2, ctx.k, ctx.n, dtype=torch.int64, device=ctx.device))
    with pytest.raises(ValueError, match="`planes`"):
        ev.channel_mix(np.ones((3, 3), dtype=np.int64), ctx.random_ct(2, 2))
    with pytest.raises(fhe.FheError, match="out of range"):
        fhe.Block8x8Plan(ctx, eye * (lim + 1), eye)


def test_cpp_host_agrees_with_the_python_host(fhe, tmp_path):
    """seal/packed_check (seal::hip::channel_mix + block8x8_scalar over the facade) on a stream of seeded ciphertexts: the bytes of
    circuits.packed_jpeg_compress"""
    import subprocess
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "packed_check")
    assert os.path.exists(exe), "build() makes seal/packed_check"
    ctx, ev = _ctx(fhe, "Q4", po.T41)
    planes = ctx.random_ct(3, 1, 64, seed=fhe.SEED + 9)
    fin, fout = str(tmp_path / "in.ct"), str(tmp_path / "out.ct")
    with open(fin, "wb") as f:
        for c in fhe.to_host(planes).reshape(-1, 2, ctx.k, ctx.n):
            fhe.server.write_ciphertext(f, c)
    want = fhe.to_host(fhe.circuits.packed_jpeg_compress(ev, fhe.circuits.packed_dct_plan(ctx), planes[0], planes[1], planes[2]))
    r = subprocess.run([exe, fin, fout, "1", "8", "8", str(ctx.n), str(ctx.t)] + [str(q) for q in ctx.q], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    fwant = str(tmp_path / "want.ct")
    with open(fwant, "wb") as f:
        for c in want.reshape(-1, 2, ctx.k, ctx.n):
            fhe.server.write_ciphertext(f, c)
    assert open(fout, "rb").read() == open(fwant, "rb").read()
    flat = want.reshape(-1)
    with np.errstate(over="ignore"):
        digest = int((flat * (np.uint64(2) * np.arange(flat.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))
    assert "digest=%016x" % digest in r.stdout, r.stdout
