"""GPU: modulus switching (include/fhe_hip.h fhe_mod_switch / fhe_ctx_create_level; csrc/modswitch.hip) against the specification
(tests/modswitch_oracle.py, whose forms tests/test_modswitch_cpu.py checks against each other): bit-exact on every base, level, size and
batch count for random residues, residues q_i - 1 and the crafted operands; one call == two calls through a level context; real
encryptions switched as far as circuits.mod_switch_primes allows decrypt to the same plaintext within the noise bound; work continues in
the level context; refusals; the streaming servers with out_primes; the C++ host.  Everything at n = 1024."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import modswitch_oracle as mo
import packed_oracle as po
from test_gpu_galois import _unreduced

pytestmark = pytest.mark.gpu

N = 1024
PRIMES = mo.bases(N)
BASES = {name: (PRIMES[name], {}) for name in ("Q3", "Q4", "Q58", "Q61", "Q61R", "S16K")}
BASES["shoup"] = (PRIMES["Q4"], {"FHE_NTT_NOPM": "1"})
_cache = {}


def _ctx(fhe, name, t=1 << 14):
    if (name, t) not in _cache:
        q, sw = BASES[name]
        ctx = fhe.SEALContext(N, q, t, switches=sw or None)
        _cache[(name, t)] = (ctx, fhe.Evaluator(ctx))
    return _cache[(name, t)]


def _inputs(fhe, ctx, name):
    """[(what, uint64 [3, 3, k, n])]: random residues, every residue at q_i - 1, and per k_out the crafted coefficient list tiled across
    every polynomial -- each with the specification's result at every level, computed once"""
    key = ("inputs", name)
    if key not in _cache:
        k = ctx.k
        items = [("random", fhe.to_host(ctx.random_ct(3, size=3, seed=fhe.SEED + k))),
                 ("top", np.broadcast_to(np.array(ctx.q, dtype=np.uint64)[None, None, :, None] - np.uint64(1), (3, 3, k, N)).copy())]
        for k_out in range(1, k):
            items.append(("crafted for k_out=%d" % k_out, np.broadcast_to(mo.crafted_tile(ctx.q, k_out, N, seed=k_out)[None, None], (3, 3, k, N)).copy()))
        _cache[key] = [(what, x, mo.switch_residues_levels(x[:1, :1] if what != "random" else x, ctx.q)) for what, x in items]
    return _cache[key]


@pytest.mark.parametrize("name", list(BASES))
def test_mod_switch_matches_the_specification(fhe, name):
    """every k_out in 1 .. k - 1, sizes 2 and 3, batch counts 1 and 3; every output word is below its prime"""
    import torch
    ctx, ev = _ctx(fhe, name)
    k = ctx.k
    print("\n[mod_switch %s k=%d] max prime %d bits, lazy products: %s" % (name, k, max(q.bit_length() for q in ctx.q),
                                                                          max(q.bit_length() for q in ctx.q) <= 58 and name != "shoup"))
    for what, x, levels in _inputs(fhe, ctx, name):
        for k_out in range(1, k):
            if what.startswith("crafted") and what != "crafted for k_out=%d" % k_out:
                continue
            lctx = ctx.level(k_out)
            assert (lctx.k, lctx.n, lctx.t, lctx.q) == (k_out, N, ctx.t, ctx.q[:k_out])
            for size in (2, 3):
                for batch in (1, 3):
                    ct = fhe.to_device(x[:batch, :size], ctx.device)
                    keep = ct.clone()
                    out = ev.mod_switch(ct, k_out)
                    assert tuple(out.shape) == (batch, size, k_out, N)
                    want = levels[k_out]
                    want = np.broadcast_to(want, (batch, size, k_out, N)) if what != "random" else want[:batch, :size]
                    assert np.array_equal(fhe.to_host(out), want), (name, what, k_out, size, batch)
                    assert _unreduced(fhe, lctx, out) == 0
                    assert torch.equal(ct, keep), "the input was written"


@pytest.mark.parametrize("name", ["Q3", "Q4", "S16K", "Q61R"])
def test_one_call_equals_two_calls_through_a_level_context(fhe, name):
    """k -> k_out == k -> k_1 followed, in ctx.level(k_1), by k_1 -> k_out, bit for bit (fhe_ctx_create_level: the child's constants are
    the parent's for its first k_1 primes)"""
    import torch
    ctx, ev = _ctx(fhe, name)
    ct = ctx.random_ct(2, size=3, seed=fhe.SEED + 17)
    for k_1 in range(2, ctx.k):
        mid_ctx = ctx.level(k_1)
        assert ctx.level(k_1) is mid_ctx                                                   # cached
        mid = ev.mod_switch(ct, k_1)
        for k_out in range(1, k_1):
            assert torch.equal(fhe.Evaluator(mid_ctx).mod_switch(mid, k_out), ev.mod_switch(ct, k_out)), (name, k_1, k_out)
    if ctx.k == 2:
        assert tuple(ev.mod_switch(ct, 1).shape) == (2, 3, 1, N)


def _client(fhe, name, t):
    key = ("client", name, t)
    if key not in _cache:
        ctx, ev = _ctx(fhe, name, t)
        kg = fhe.KeyGenerator(ctx, seed=31)
        _cache[key] = (ctx, ev, kg, fhe.DeviceEncryptor(ctx, kg.public_key(), key=bytes(range(32)), reproducible=True), fhe.Decryptor(ctx, kg.secret_key()),
                       fhe.BatchEncoder(ctx))
    return _cache[key]


@pytest.mark.parametrize("name,t", [("Q4", po.T33), ("Q3", 65537)])
def test_real_encryptions_keep_their_plaintext_and_the_bound(fhe, name, t):
    """batch-encoded random slots, one multiply_plain by a scalar, switched to every level mod_switch_primes(keep_bits=4) allows: the level
    Decryptor gives the top-level plaintext; the reported budget (a difference of two bit lengths, within +-1 of the true value) is at
    least floor(bound) - 1 with the bound computed from the reported input budget minus 1 -- no other slack"""
    ctx, ev, kg, enc, dec, be = _client(fhe, name, t)
    c = fhe.circuits
    rng = np.random.default_rng(5)
    slots = rng.integers(0, t, size=(2, N), dtype=np.uint64)
    enc.seek(0)
    ct = ev.multiply_plain(enc.encrypt_plains(be.encode(slots)), np.array([12345], dtype=np.uint64))
    plain, budgets = dec.decrypt_batch(ct, with_budget=True)
    assert np.array_equal(be.decode(plain).astype(object), slots.astype(object) * 12345 % t)
    budget = min(budgets)
    lowest = c.mod_switch_primes(ctx, budget - 1, 4)
    assert lowest < ctx.k, "no level qualifies: %d bits" % budget
    report = []
    for k_out in range(ctx.k - 1, lowest - 1, -1):
        lctx = ctx.level(k_out)
        ldec = fhe.Decryptor(lctx, kg.secret_key()[:k_out].contiguous())
        got, lb = ldec.decrypt_batch(ev.mod_switch(ct, k_out), with_budget=True)
        bound = c.mod_switch_budget(ctx, budget - 1, k_out)
        report.append("%d primes: %d bits (bound %.1f)" % (k_out, min(lb), bound))
        assert np.array_equal(got, plain), (name, k_out)
        assert min(lb) >= math.floor(bound) - 1, (name, report)
    print("\n[mod_switch %s t=%d] %d bits at %d primes -> %s" % (name, t, budget, ctx.k, "; ".join(report)))
    assert lowest == 1 or c.mod_switch_budget(ctx, budget - 1, lowest - 1) < 4


def test_work_continues_in_the_level_context(fhe):
    """Q4, t = T33, switched 4 -> 2: add, multiply_plain, one plane_map and one rotate_rows (Galois keys generated in the level context for
    the same secret key) decrypt to the expected slots"""
    ctx, ev, kg, enc, dec, be = _client(fhe, "Q4", po.T33)
    t, k_out = ctx.t, 2
    rng = np.random.default_rng(9)
    slots = rng.integers(0, 1000, size=(3, N), dtype=np.uint64)
    enc.seek(100)
    low = ev.mod_switch(enc.encrypt_plains(be.encode(slots)), k_out)
    lctx = ctx.level(k_out)
    sk = kg.secret_key()[:k_out].contiguous()
    lev, ldec, lbe = fhe.Evaluator(lctx), fhe.Decryptor(lctx, sk), fhe.BatchEncoder(lctx)
    val = lambda x: lbe.decode(ldec.decrypt_batch(x)).astype(object)
    s = slots.astype(object)
    assert np.array_equal(val(low), s)
    assert np.array_equal(val(lev.add(low[:1], low[1:2])), (s[:1] + s[1:2]) % t)
    assert np.array_equal(val(lev.multiply_plain(low, np.array([77], dtype=np.uint64))), s * 77 % t)
    taps, w = np.array([[0, 2], [1, 1]], dtype=np.uint32), np.array([[3, -5], [7, 0]], dtype=np.int64)
    got = val(lev.plane_map(fhe.PlaneMapPlan(lctx, 3, taps, w), low[None])[0])
    assert np.array_equal(got, np.stack([(3 * s[0] - 5 * s[2]) % t, 7 * s[1] % t]))
    lkg = fhe.KeyGenerator(lctx, seed=32, secret_key=sk)
    assert bool((lkg.secret_key() == sk).all())
    gk = lkg.generate_galois_keys(30, elements=[fhe.galois_element(N, 1)])
    rot, budget = ldec.decrypt_batch(lev.rotate_rows(low[:1], 1, gk), with_budget=True)
    half = N // 2
    want = np.concatenate([np.roll(slots[0, :half], -1), np.roll(slots[0, half:], -1)])
    assert np.array_equal(lbe.decode(rot)[0], want) and budget[0] > 0
    # the level key generator's public key encrypts for the same secret key
    fresh = fhe.DeviceEncryptor(lctx, lkg.public_key()).encrypt_plains(lbe.encode(slots[:1]))
    assert np.array_equal(val(fresh), s[:1])


def test_refusals(fhe):
    """each case of the specification is FHE_ERR_PARAM with fhe_last_error() set before anything is enqueued: the output keeps its sentinel"""
    import torch
    ctx, ev = _ctx(fhe, "Q3")
    L = fhe._lib.load()
    k, n = ctx.k, ctx.n
    buf = torch.full((4 * 2 * k * n + 4 * 2 * (k - 1) * n + 64,), -1, dtype=torch.int64, device=ctx.device)
    in_words = 4 * 2 * k * n
    buf[:in_words].copy_(ctx.random_ct(4).reshape(-1))
    at = lambda words: C.c_void_p(buf.data_ptr() + 8 * words)

    def run(c=ctx.h, k_out=k - 1, src=at(0), dst=at(in_words), n_polys=8):
        return L.fhe_mod_switch(c, k_out, src, dst, n_polys, None)
    for bad in (0, k, k + 1, 9):
        assert run(k_out=bad) == -1 and b"k_out" in L.fhe_last_error(), bad
    assert run(c=None) == -1 and run(src=None) == -1 and run(dst=None) == -1 and b"null" in L.fhe_last_error()
    out_words = 8 * (k - 1) * n
    for dst in (at(0), at(n), at(in_words - 1), at(in_words - out_words + 1)):              # the input itself, inside it, its last word
        assert run(dst=dst) == -1 and b"overlaps" in L.fhe_last_error()
    assert run(src=at(1), dst=at(in_words)) == -1 and b"overlaps" in L.fhe_last_error()     # an input that ends inside the output
    assert run(src=at((k - 1) * n - 1), dst=at(0), n_polys=1) == -1                         # an output that ends inside the input
    assert run(n_polys=0) == 0
    h = C.c_void_p()
    for bad in (0, k, k + 1):
        assert L.fhe_ctx_create_level(ctx.h, bad, C.byref(h)) == -1 and not h.value and b"k_out" in L.fhe_last_error()
    assert L.fhe_ctx_create_level(None, 1, C.byref(h)) == -1 and L.fhe_ctx_create_level(ctx.h, 1, None) == -1
    torch.cuda.synchronize()
    assert bool((buf[in_words:] == -1).all()), "a refused call wrote its output"
    assert run() == 0                                                                        # adjacent ranges do not overlap
    torch.cuda.synchronize()
    assert bool((buf[in_words + out_words:] == -1).all()) and not bool((buf[in_words:in_words + out_words] == -1).any())
    single = fhe.SEALContext(N, ctx.q[:1], ctx.t)
    assert L.fhe_mod_switch(single.h, 1, at(0), at(in_words), 1, None) == -1                 # one prime: nothing to drop
    with pytest.raises(ValueError, match="k_out"):
        ev.mod_switch(ctx.random_ct(1), k)
    with pytest.raises(ValueError, match="`ct`"):
        ev.mod_switch(ctx.level(2).random_ct(1), 1)
    with pytest.raises(ValueError, match="`out`"):
        ev.mod_switch(ctx.random_ct(1), 2, out=ctx.empty(1))
    with pytest.raises(ValueError, match="out_primes"):
        fhe.server._out_level(ctx, k)
    with pytest.raises(fhe.FheError):
        ctx.level(k)


@pytest.mark.parametrize("w,h,dw,dh,bits,rows_per_step", [(5, 9, 3, 4, 6, 1), (3, 16, 4, 48, None, 5)])
def test_server_resize_plain_with_out_primes(fhe, tmp_path, w, h, dw, dh, bits, rows_per_step):
    """out_primes = k - 1: the output file is exactly records x (header + 2 k_out n 8) bytes, its records are the mod-switched records of
    the unswitched run, and the client -- level context, level Decryptor -- decodes the values of the unswitched run"""
    ctx, ev = _ctx(fhe, "Q3")
    k_out = ctx.k - 1
    kg = fhe.KeyGenerator(ctx, seed=23)
    enc = fhe.FractionalEncoder(ctx)
    rgb = np.random.default_rng(w * h + dh).integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    fin, fout, flow = (str(tmp_path / x) for x in ("in.ct", "out.ct", "low.ct"))
    assert fhe.client.send_resize(ctx, fhe.DeviceEncryptor(ctx, kg.public_key()), enc, rgb, fin) == (w, h)
    kw = dict(weight_bits=bits, rows_per_step=rows_per_step)
    assert fhe.server.server_resize_plain(ctx, fin, fout, w, h, dw, dh, "catmull_rom", **kw) == dw * dh
    stats = {}
    assert fhe.server.server_resize_plain(ctx, fin, flow, w, h, dw, dh, "catmull_rom", out_primes=k_out, stats=stats, **kw) == dw * dh
    records = dw * dh * 3
    assert os.path.getsize(fout) == records * (fhe.server.RECORD_HEADER + 2 * ctx.k * N * 8)
    assert os.path.getsize(flow) == records * (fhe.server.RECORD_HEADER + 2 * k_out * N * 8) == stats["bytes_out"]
    lctx = ctx.level(k_out)
    full = np.zeros((records, 2, ctx.k, N), dtype=np.uint64)
    low = np.zeros((records, 2, k_out, N), dtype=np.uint64)
    with open(fout, "rb") as f, open(flow, "rb") as g:
        for i in range(records):
            fhe.server.read_ciphertext_into(f, full[i])
            fhe.server.read_ciphertext_into(g, low[i])
        assert g.read(1) == b""
    assert np.array_equal(low, fhe.to_host(ev.mod_switch(fhe.to_device(full, ctx.device), k_out)))
    a, b = [], []
    fhe.client.receive_pixels(ctx, fhe.Decryptor(ctx, kg.secret_key()), enc, fout, dw, dh, decoded=a)
    px = fhe.client.receive_pixels(lctx, fhe.Decryptor(lctx, kg.secret_key()[:k_out].contiguous()), fhe.FractionalEncoder(lctx), flow, dw, dh, decoded=b)
    assert a == b and px.shape == (dh, dw, 3)


def test_server_jpeg_with_out_primes(fhe, tmp_path):
    """one 8x8 colour block at n = 1024, the P4096 primes: server_jpeg with out_primes = k - 1 writes 192 records of k_out primes whose
    decrypted, rounded coefficients are those of the unswitched run; server_jpeg_decompress takes the same argument"""
    ctx, ev = _ctx(fhe, "Q3")
    k_out = ctx.k - 1
    kg = fhe.KeyGenerator(ctx, seed=24)
    enc = fhe.FractionalEncoder(ctx)
    rgb = np.random.default_rng(3).integers(0, 256, size=(8, 8, 3)).astype(np.uint8)
    fin, fout, flow, fback = (str(tmp_path / x) for x in ("in.ct", "out.ct", "low.ct", "back.ct"))
    assert fhe.client.send_jpeg(ctx, fhe.DeviceEncryptor(ctx, kg.public_key()), enc, rgb, fin) == 1
    quant = list(fhe.YQT)
    assert fhe.server.server_jpeg(ctx, fin, fout, 1, quant=quant) == 1
    stats = {}
    assert fhe.server.server_jpeg(ctx, fin, flow, 1, quant=quant, out_primes=k_out, stats=stats) == 1
    assert os.path.getsize(fout) == 192 * (fhe.server.RECORD_HEADER + 2 * ctx.k * N * 8) == stats["bytes_in"]
    assert os.path.getsize(flow) == 192 * (fhe.server.RECORD_HEADER + 2 * k_out * N * 8) == stats["bytes_out"]
    lctx = ctx.level(k_out)
    want = fhe.client.receive_jpeg(ctx, fhe.Decryptor(ctx, kg.secret_key()), enc, fout, 8, 8, str(tmp_path / "a.jpg"))
    got = fhe.client.receive_jpeg(lctx, fhe.Decryptor(lctx, kg.secret_key()[:k_out].contiguous()), fhe.FractionalEncoder(lctx), flow, 8, 8, str(tmp_path / "b.jpg"))
    assert len(got) == 1 and np.array_equal(got[0], want[0]) and np.any(want[0] != 0)
    assert fhe.server.server_jpeg_decompress(ctx, fout, fback, 1, quant=quant, out_primes=k_out) == 1
    assert os.path.getsize(fback) == 192 * (fhe.server.RECORD_HEADER + 2 * k_out * N * 8)


def test_cpp_host_agrees_with_the_python_host(fhe, tmp_path):
    """seal/modswitch_check (seal::hip::level_context + mod_switch over the facade) on a stream of seeded ciphertexts: the bytes and the
    digest of Evaluator.mod_switch"""
    import subprocess
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "modswitch_check")
    assert os.path.exists(exe), "build() makes seal/modswitch_check"
    ctx, ev = _ctx(fhe, "Q4")
    count, size, k_out = 5, 3, 2
    ct = ctx.random_ct(count, size=size, seed=fhe.SEED + 9)
    fin, fout, fwant = (str(tmp_path / x) for x in ("in.ct", "out.ct", "want.ct"))
    with open(fin, "wb") as f:
        for c in fhe.to_host(ct):
            fhe.server.write_ciphertext(f, c)
    want = fhe.to_host(ev.mod_switch(ct, k_out))
    r = subprocess.run([exe, fin, fout, str(count), str(size), str(k_out), str(N), str(ctx.t)] + [str(q) for q in ctx.q], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(fwant, "wb") as f:
        for c in want:
            fhe.server.write_ciphertext(f, c)
    assert open(fout, "rb").read() == open(fwant, "rb").read()
    flat = want.reshape(-1)
    with np.errstate(over="ignore"):
        digest = int((flat * (np.uint64(2) * np.arange(flat.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))
    m = re.search(r"digest=([0-9a-f]{16})", r.stdout)
    assert m and int(m.group(1), 16) == digest, r.stdout
