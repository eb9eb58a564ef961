"""GPU: seeded symmetric encryption (include/fhe_hip.h fhe_expand_seeded / fhe_seed_expand_a / fhe_encrypt_symmetric_batch,
csrc/encrypt.hip k_seed_expand / k_enc_sym_fused and the composition of launches) against the Python-integer model of
tests/seeded_oracle.py, bit for bit, and through client.send_jpeg -> server_jpeg(seeded=...) -> client.receive_jpeg.  Everything at
n = 1024: one wave per polynomial in the fused kernel, 256 cipher blocks per residue row in the expansion."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import seeded_oracle as so

pytestmark = pytest.mark.gpu
N = 1024
A_KEY, N_KEY = bytes(range(32)), bytes(range(100, 132))
M64 = (1 << 64) - 1
FIRSTS = (0, (1 << 40) + 3, (1 << 64) - 2)                     # a batch of 5 from 2^64 - 2 wraps
ERR_PARAM = -1


@functools.lru_cache(maxsize=None)
def _bases():
    """label -> (q, t, arithmetic of fhe_encrypt_symmetric_batch), the pairs of tests/test_gpu_encrypt.py: pseudo-Mersenne class 1 -> EncPmA,
    class 2 -> EncPmB, no class and primes of 34 .. 58 bits -> EncShoup, 59 .. 61-bit primes -> the composition of launches"""
    import decrypt_craft as dc
    from oracle.oracle import PRESETS
    from packed_oracle import T41
    return {"P4096": (tuple(PRESETS["P4096"]["q"]), 1 << 14, "EncShoup"), "Q4-k3": (tuple(dc.primes("Q4", 3)), 65537, "EncPmA"),
            "W58": (tuple(dc.primes("W58", 2)), T41, "EncPmB"), "W61": (tuple(dc.primes("W61", 2)), (1 << 59) + 1, "composed"),
            "K8": (tuple(PRESETS["SEAL23_16384"]["q"]), 1 << 14, "EncPmA")}


LABELS = ["P4096", "Q4-k3", "W58", "W61", "K8"]


@functools.lru_cache(maxsize=None)
def _model_a(label, first):
    """[5, k, n]: the model's expansion of ciphertexts first .. first + 4 (mod 2^64); computed once, shared, never written"""
    a = so.expand_batch(_bases()[label][0], N, A_KEY, first, 5)
    a.setflags(write=False)
    return a


def _expand_a(fhe, ctx, count, first, key=A_KEY):
    out = torch.empty((count, ctx.k, ctx.n), dtype=torch.int64, device=ctx.device)
    fhe._lib.call("fhe_seed_expand_a", ctx.h, count, key, first, C.c_void_p(out.data_ptr()), None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("label", LABELS)
def test_expansion_equals_the_model_bit_for_bit(fhe, label):
    q, t, _ = _bases()[label]
    ctx = fhe.SEALContext(N, q, t)
    ev = fhe.Evaluator(ctx)
    assert [p.bit_length() for p in q] == {"P4096": [36, 36, 37], "Q4-k3": [55, 55, 54], "W58": [58, 58], "W61": [61, 61], "K8": [55] * 6 + [54] * 2}[label]
    for first in FIRSTS:
        want = _model_a(label, first)
        for count in (1, 5):
            c0 = ctx.random_ct(count, size=1, seed=11 + count)[:, 0].contiguous()
            keep = c0.clone()
            got = ev.expand_seeded(c0, A_KEY, first)
            assert tuple(got.shape) == (count, 2, ctx.k, N) and torch.equal(c0, keep)
            assert torch.equal(got[:, 0], keep), (label, first, count)                         # c0 arrives untouched in polynomial 0
            assert np.array_equal(fhe.to_host(got[:, 1]), want[:count]), (label, first, count)
            assert np.array_equal(fhe.to_host(_expand_a(fhe, ctx, count, first)), want[:count])
        # [0, 5) = [0, 2) followed by [2, 5), also across the wrap
        parts = torch.cat([_expand_a(fhe, ctx, 2, first), _expand_a(fhe, ctx, 3, (first + 2) & M64)])
        assert np.array_equal(fhe.to_host(parts), want)
        # the level context's expansion is the prefix of this one
        low = ctx.level(ctx.k - 1)
        assert np.array_equal(fhe.to_host(_expand_a(fhe, low, 5, first)), want[:, :ctx.k - 1])
    assert not np.array_equal(fhe.to_host(_expand_a(fhe, ctx, 1, 0, key=N_KEY)), _model_a(label, 0)[:1])


def test_expansion_beyond_one_trip_of_the_grid_stride_loop(fhe):
    """k_seed_expand runs at most 8,192 workgroups of 256 threads = 2,097,152 cipher blocks per trip of its loop; 3,000 ciphertexts of
    3 x 1024 residues are 2,304,000 blocks: the tail is produced by the second trip.  A 64-ciphertext prefix against the model, the whole
    against the same data made in two calls (each within one trip), by fhe_digest and word for word."""
    q, t, _ = _bases()["P4096"]
    ctx = fhe.SEALContext(N, q, t)
    count, first = 3000, (1 << 40) + 3
    assert count * ctx.k * (N // 4) > 8192 * 256 > (count // 2) * ctx.k * (N // 4)
    whole = _expand_a(fhe, ctx, count, first)
    two = torch.cat([_expand_a(fhe, ctx, count // 2, first), _expand_a(fhe, ctx, count - count // 2, first + count // 2)])
    assert ctx.digest(whole) == ctx.digest(two) and torch.equal(whole, two)
    assert np.array_equal(fhe.to_host(whole[:64]), so.expand_batch(q, N, A_KEY, first, 64))
    tail = fhe.to_host(whole[count - 1])
    assert np.array_equal(tail, so.expand_a(q, N, A_KEY, first + count - 1))


def _rows(t):
    thr = (t + 1) >> 1
    row = np.array([0, 1, thr - 2, thr - 1, thr, thr + 1, t - 2, t - 1] * (N // 8), dtype=np.uint64)
    np.random.default_rng(23).shuffle(row)
    return np.stack([row, np.full(N, t - 1, dtype=np.uint64), np.full(N, thr, dtype=np.uint64)])


@pytest.mark.parametrize("label", LABELS)
def test_symmetric_encryption_equals_the_model_and_decrypts(fhe, oracle_mod, label):
    """fhe_encrypt_symmetric_batch: the one-launch kernel (built for two and for four waves per SIMD) == the composition of launches
    (FHE_SYM_UNFUSED=1) == the model, bit for bit; the phase under the oracle is Delta m' - e exactly; the expanded ciphertext decrypts to its
    plaintext with the oracle's noise figure, with no less budget than fhe_encrypt_batch leaves; the same in the level context."""
    q, t, arith = _bases()[label]
    ctx, orc = fhe.SEALContext(N, q, t), oracle_mod.Oracle(N, q, t)
    pm_class, bits = fhe._lib.call("fhe_arith_path", ctx.h) & 3, [p.bit_length() for p in q]      # what fhe_encrypt_symmetric_batch dispatches on
    assert pm_class == {"EncPmA": 1, "EncPmB": 2}.get(arith, 0), (label, pm_class, arith)
    assert arith != "EncShoup" or (max(bits) <= 58 and min(bits) >= 34)
    assert arith != "composed" or max(bits) > 58
    kg = fhe.KeyGenerator(ctx, seed=17)
    sk_dev = kg.secret_key()
    sk = fhe.to_host(sk_dev)
    plains = _rows(t)
    first = (1 << 35) + 3
    outs, zeros = [], []
    for sw in ({}, {"FHE_ENC_OCC": 4}, {"FHE_SYM_UNFUSED": 1}):
        c2 = fhe.SEALContext(N, q, t, switches=sw) if sw else ctx
        enc = fhe.SymmetricEncryptor(c2, sk_dev, a_key=A_KEY, noise_key=N_KEY, reproducible=True)
        enc.seek(first)
        s = enc.encrypt_plains(fhe.to_device(plains, ctx.device))
        assert (s.a_key, s.first_index, len(s), enc.next) == (A_KEY, first, 3, first + 3)
        outs.append(s.c0)
        zeros.append(enc.encrypt_zeros(3).c0)                                                   # d_plain = NULL, indices first + 3 ..
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2]), label               # fused == composition
    assert torch.equal(zeros[0], zeros[2]) and torch.equal(zeros[1], zeros[2]), label
    ev, dec = fhe.Evaluator(ctx), fhe.Decryptor(ctx, sk_dev)
    c0s = torch.cat([outs[0], zeros[0]])
    rows = np.concatenate([plains, np.zeros((3, N), dtype=np.uint64)])
    full = ev.expand_seeded(c0s, A_KEY, first)
    back, budgets = dec.decrypt_batch(full, with_budget=True)
    assert np.array_equal(back, rows)
    host = fhe.to_host(full)
    pk_enc = fhe.DeviceEncryptor(ctx, kg.public_key(), key=N_KEY, reproducible=True)
    pk_enc.seek(first)
    _, pk_budgets = dec.decrypt_batch(pk_enc.encrypt_plains(fhe.to_device(rows, ctx.device)), with_budget=True)
    for i in range(6):
        c0, a = so.encrypt(orc, sk, rows[i], A_KEY, N_KEY, first + i)
        assert np.array_equal(host[i, 1], a) and np.array_equal(host[i, 0], c0), (label, i)
        assert np.array_equal(orc.decrypt_phase(sk, host[i]), so.target_phase(orc, rows[i], N_KEY, first + i)), (label, i)
        want, nb, mb = orc.decrypt_noise_bits(sk, host[i])
        assert np.array_equal(want, rows[i]) and budgets[i] == max(0, mb - nb - 1) and budgets[i] > 0, (label, i, budgets[i], nb, mb)
        assert budgets[i] >= pk_budgets[i], (label, i, budgets[i], pk_budgets[i])               # e alone against e u + e1 + e2 s
    # the level context, with sk[:k - 1]: what a client of the special-prime pipelines encrypts in
    low, k1 = ctx.level(ctx.k - 1), ctx.k - 1
    sk_low = sk_dev[:k1].contiguous()
    lenc = fhe.SymmetricEncryptor(low, sk_low, a_key=A_KEY, noise_key=N_KEY, reproducible=True)
    lenc.seek(first)
    ls = lenc.encrypt_plains(fhe.to_device(plains, ctx.device))
    lfull = ls.expand(fhe.Evaluator(low))
    lback, lbud = fhe.Decryptor(low, sk_low).decrypt_batch(lfull, with_budget=True)
    lorc = oracle_mod.Oracle(N, q[:k1], t)
    lhost = fhe.to_host(lfull)
    for i in range(3):
        want, nb, mb = lorc.decrypt_noise_bits(sk[:k1].copy(), lhost[i])
        assert np.array_equal(lback[i], want) and lbud[i] == max(0, mb - nb - 1), (label, i)
    # With Delta = floor(q / t) the invariant noise of a fresh symmetric ciphertext is t |e| + (q mod t) |m centred| <= 19 t + t^2 / 2 < t^2
    # (|e| <= 19, these rows hold coefficients up to t / 2 in size): below q / 2, so that it decrypts, whenever the level's q exceeds 2 t^2.
    # The single 58-bit prime left under t = T41 and the single 61-bit prime under t = 2^59 + 1 do not: those levels hold no dense plaintext,
    # whoever encrypts, and what is checked there is that device and oracle agree on every bit and on the noise figure (above).
    q_low = 1
    for p in q[:k1]:
        q_low *= p
    if q_low > 2 * t * t:
        assert np.array_equal(lback, plains) and min(lbud) > 0, label
    else:
        assert label in ("W58", "W61")
    lc0, la = so.encrypt(lorc, sk[:k1].copy(), plains[0], A_KEY, N_KEY, first)
    assert np.array_equal(fhe.to_host(lfull[0]), np.stack([lc0, la]))
    assert np.array_equal(la, fhe.to_host(full[0, 1, :k1]))                                     # the same a as in the parent


def test_encryptor_key_discipline(fhe):
    q, t, _ = _bases()["P4096"]
    ctx = fhe.SEALContext(N, q, t)
    kg = fhe.KeyGenerator(ctx, seed=2)
    enc = fhe.SymmetricEncryptor(ctx, kg.secret_key())               # both keys from the OS generator
    assert enc.seeded is True
    with pytest.raises(RuntimeError):
        enc.seek(0)                                                  # would allow an (a_key, index) pair to repeat
    a, b = enc.encrypt_zeros(2), enc.encrypt_zeros(2)
    assert (a.first_index, b.first_index, enc.next) == (0, 2, 4) and not torch.equal(a.c0, b.c0)
    assert fhe.SymmetricEncryptor(ctx, kg.secret_key()).a_key != enc.a_key
    keyed = fhe.SymmetricEncryptor(ctx, kg.secret_key(), a_key=A_KEY, noise_key=N_KEY)      # a caller's own keys WITHOUT reproducible=True
    keyed.encrypt_zeros(1)
    with pytest.raises(RuntimeError):
        keyed.seek(0)
    with pytest.raises(ValueError):
        fhe.SymmetricEncryptor(ctx, kg.secret_key(), a_key=A_KEY, reproducible=True)        # reproducible needs both keys
    with pytest.raises(ValueError):
        fhe.SymmetricEncryptor(ctx, kg.secret_key(), a_key=b"short")
    vals = [0.0, 1.5, -2.25, 100.0]
    s = keyed.encrypt_values(vals)
    fe = fhe.FractionalEncoder(ctx)
    plains = fhe.Decryptor(ctx, kg.secret_key()).decrypt_batch(s.expand(fhe.Evaluator(ctx)))
    assert [fe.decode(p) for p in plains] == vals and s.first_index == 1


def test_refusals_leave_the_outputs_untouched(fhe):
    q, t, _ = _bases()["P4096"]
    ctx = fhe.SEALContext(N, q, t)
    k, w = ctx.k, ctx.k * N
    kg = fhe.KeyGenerator(ctx, seed=5)
    enc = fhe.SymmetricEncryptor(ctx, kg.secret_key(), a_key=A_KEY, noise_key=N_KEY)
    skn = enc._sk_ntt
    lib = fhe._lib.load()
    p = lambda x: C.c_void_p(x.data_ptr())
    flat = torch.full((4 * w,), 0x5A5A5A5A, dtype=torch.int64, device=ctx.device)
    c0 = ctx.random_ct(1, size=1, seed=3).reshape(-1)
    scratch = torch.full((w,), 0x5A5A5A5A, dtype=torch.int64, device=ctx.device)
    untouched = lambda x: bool((x == 0x5A5A5A5A).all())
    # fhe_expand_seeded: null pointers, overlapping ranges (from either side)
    assert lib.fhe_expand_seeded(None, p(c0), 1, A_KEY, 0, p(flat), None) == ERR_PARAM
    assert lib.fhe_expand_seeded(ctx.h, None, 1, A_KEY, 0, p(flat), None) == ERR_PARAM
    assert lib.fhe_expand_seeded(ctx.h, p(c0), 1, None, 0, p(flat), None) == ERR_PARAM
    assert lib.fhe_expand_seeded(ctx.h, p(c0), 1, A_KEY, 0, None, None) == ERR_PARAM
    assert lib.fhe_expand_seeded(ctx.h, p(flat[w // 2:]), 1, A_KEY, 0, p(flat), None) == ERR_PARAM and b"overlap" in lib.fhe_last_error()
    assert lib.fhe_expand_seeded(ctx.h, p(flat), 1, A_KEY, 0, p(flat[w // 2:]), None) == ERR_PARAM
    assert lib.fhe_expand_seeded(ctx.h, p(flat[2 * w - 2:]), 1, A_KEY, 0, p(flat), None) == ERR_PARAM          # the last two words of d_out
    assert lib.fhe_seed_expand_a(ctx.h, 1, None, 0, p(flat), None) == ERR_PARAM
    assert lib.fhe_seed_expand_a(ctx.h, 1, A_KEY, 0, None, None) == ERR_PARAM
    # fhe_encrypt_symmetric_batch: null pointers, short scratch, an index that would wrap
    need = lib.fhe_encrypt_symmetric_scratch_bytes(ctx.h, 2)
    assert need == 2 * w * 8
    args = lambda **kw: [kw.get("ctx", ctx.h), kw.get("sk", p(skn)), None, 2, kw.get("ak", A_KEY), kw.get("nk", N_KEY), kw.get("first", 0), kw.get("out", p(flat)),
                         kw.get("scratch", p(flat[2 * w:])), kw.get("bytes", need), None]
    for bad in (dict(ctx=None), dict(sk=None), dict(ak=None), dict(nk=None), dict(out=None), dict(scratch=None), dict(bytes=need - 8), dict(bytes=0),
                dict(first=M64)):
        assert lib.fhe_encrypt_symmetric_batch(*args(**bad)) == ERR_PARAM, bad
    torch.cuda.synchronize()
    assert untouched(flat) and untouched(scratch)
    # count = 0 is a no-op that succeeds, whatever the pointers
    assert lib.fhe_expand_seeded(ctx.h, None, 0, A_KEY, 0, None, None) == 0
    assert lib.fhe_seed_expand_a(ctx.h, 0, A_KEY, 0, None, None) == 0
    assert lib.fhe_encrypt_symmetric_batch(ctx.h, p(skn), None, 0, A_KEY, N_KEY, 0, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert untouched(flat)
    assert len(enc.encrypt_zeros(0)) == 0 and tuple(fhe.Evaluator(ctx).expand_seeded(ctx.empty(0, size=1)[:, 0].contiguous(), A_KEY, 0).shape) == (0, 2, k, N)
    # adjacent ranges do not overlap: the same call goes through
    assert lib.fhe_expand_seeded(ctx.h, p(flat[2 * w:]), 1, A_KEY, 0, p(flat), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(flat[:w], flat[2 * w:3 * w]) and not untouched(flat[w:2 * w])


@pytest.mark.parametrize("out_primes", [None, 2])
def test_seeded_stream_through_the_jpeg_server(fhe, tmp_path, out_primes):
    """A 16 x 8 image (two blocks) sent with a reproducible SymmetricEncryptor: the stream is 2 * 192 one-polynomial records and a 40-byte
    sidecar; server_jpeg(seeded="sidecar") writes byte for byte what server_jpeg writes for the same ciphertexts expanded and stored as full
    records; receive_jpeg decrypts both to the same coefficients; a c0 with one residue equal to its modulus is refused."""
    q, t, _ = _bases()["P4096"]
    ctx = fhe.SEALContext(N, q, t)
    lib = fhe._lib.load()
    kg = fhe.KeyGenerator(ctx, seed=24)
    fe = fhe.FractionalEncoder(ctx)
    rgb = np.random.default_rng(3).integers(0, 256, size=(8, 16, 3)).astype(np.uint8)
    fseed, ffull, oseed, ofull, obad = (str(tmp_path / x) for x in ("seeded.ct", "full.ct", "out_seeded.ct", "out_full.ct", "out_bad.ct"))
    first = (1 << 33) + 5
    enc = fhe.SymmetricEncryptor(ctx, kg.secret_key(), a_key=A_KEY, noise_key=N_KEY, reproducible=True)
    enc.seek(first)
    assert fhe.client.send_jpeg(ctx, enc, fe, rgb, fseed) == 2
    rec1, rec2 = lib.fhe_io_record_bytes(1, ctx.k, N), lib.fhe_io_record_bytes(2, ctx.k, N)
    assert os.path.getsize(fseed) == 2 * 192 * rec1 and os.path.getsize(fseed + ".seed") == 40
    assert fhe.client.read_seed(fseed + ".seed") == (A_KEY, first) and enc.next == first + 384
    # the same ciphertexts, expanded and stored as full records
    c0 = np.zeros((384, 1, ctx.k, N), dtype=np.uint64)
    with open(fseed, "rb") as f:
        for r in c0:
            fhe.server.read_ciphertext_into(f, r)
    full = fhe.to_host(fhe.Evaluator(ctx).expand_seeded(fhe.to_device(c0[:, 0], ctx.device), A_KEY, first))
    with open(ffull, "wb") as f:
        for ct in full:
            fhe.server.write_ciphertext(f, ct)
    assert os.path.getsize(ffull) == 384 * rec2
    quant = list(fhe.YQT)
    s_seed, s_full = {}, {}
    assert fhe.server.server_jpeg(ctx, fseed, oseed, 2, wave_blocks=1, quant=quant, out_primes=out_primes, seeded="sidecar", stats=s_seed) == 2
    assert fhe.server.server_jpeg(ctx, ffull, ofull, 2, wave_blocks=1, quant=quant, out_primes=out_primes, stats=s_full) == 2
    assert open(oseed, "rb").read() == open(ofull, "rb").read()
    assert s_seed["bytes_in"] == 384 * rec1 and s_full["bytes_in"] == 384 * rec2 and s_seed["bytes_out"] == s_full["bytes_out"]
    assert fhe.server.server_jpeg(ctx, fseed, obad, 2, quant=quant, out_primes=out_primes, seeded=(A_KEY, first)) == 2      # the pair given directly, one wave
    assert open(obad, "rb").read() == open(ofull, "rb").read()
    octx = ctx if out_primes is None else ctx.level(out_primes)
    sk = kg.secret_key() if out_primes is None else kg.secret_key()[:out_primes].contiguous()
    dec, ofe = fhe.Decryptor(octx, sk), fhe.FractionalEncoder(octx)
    got = fhe.client.receive_jpeg(octx, dec, ofe, oseed, 16, 8, str(tmp_path / "a.jpg"))
    want = fhe.client.receive_jpeg(octx, dec, ofe, ofull, 16, 8, str(tmp_path / "b.jpg"))
    assert len(got) == 2 and all(np.array_equal(g, w) for g, w in zip(got, want)) and np.any(got[0] != 0) and np.any(got[1] != 0)
    # and they are the coefficients of the same image sent under the public key
    fpk, opk = str(tmp_path / "pk.ct"), str(tmp_path / "out_pk.ct")
    fhe.client.send_jpeg(ctx, fhe.DeviceEncryptor(ctx, kg.public_key()), fe, rgb, fpk)
    assert fhe.server.server_jpeg(ctx, fpk, opk, 2, quant=quant, out_primes=out_primes) == 2
    ref = fhe.client.receive_jpeg(octx, dec, ofe, opk, 16, 8, str(tmp_path / "c.jpg"))
    assert all(np.array_equal(g, w) for g, w in zip(got, ref))
    if out_primes is None:
        # one residue of one c0 equal to its modulus: refused as the unseeded server refuses it, the output left empty
        c0[200, 0, 2, 77] = ctx.q[2]
        with open(fseed, "wb") as f:
            for r in c0:
                fhe.server.write_ciphertext(f, r)
        with pytest.raises(ValueError, match="not reduced"):
            fhe.server.server_jpeg(ctx, fseed, obad, 2, quant=quant, seeded="sidecar")
        assert os.path.getsize(obad) == 0
        with pytest.raises(EOFError):                                # a seeded stream read as full records is too short
            fhe.server.server_jpeg(ctx, fseed, obad, 2, quant=quant)
        with pytest.raises(ValueError):
            fhe.server.server_jpeg(ctx, fseed, obad, 2, quant=quant, seeded="elsewhere")
