"""Seeded symmetric encryption (include/fhe_hip.h "seeded symmetric encryption") as a Python-integer model over what
the CPU oracle already exports: the cipher block (oracle.chacha20_block), the keyed noise draw (Oracle.encrypt_draws), the lift of
add_plain and the phase (Oracle.decrypt_phase).  The reference for every bit of tests/test_seeded_cpu.py and tests/test_gpu_seeded.py.

    a_i[j]  = int.from_bytes(stream(a_key, nonce = index)[16 (i n + j) : 16 (i n + j) + 16], "little") % q_i
    e_j     = Oracle.encrypt_draws(noise_key, index)[1][j]          (the e1 draw of the public-key sampler)
    c0      = the one polynomial with  decrypt_phase(sk, (c0, a)) == Delta m' - e  in every residue

Delta m' is the lift of add_plain / k_enc_finish (delta m, + q mod t from the threshold up): `delta_lift` takes it from Oracle.add_plain on a
zero ciphertext.  (Oracle.plain_lift is the OTHER lift, multiply_plain's m + (q - t): not the one a ciphertext carries.)"""
import numpy as np

from oracle import oracle as om

M64 = (1 << 64) - 1


def expand_a(q, n, key, index):
    """[k, n] uint64: the expansion of (key, index) for the primes q, coefficient form"""
    q = [int(x) for x in q]
    index = int(index) & M64
    out = np.zeros((len(q), n), dtype=np.uint64)
    for i, qi in enumerate(q):
        for b in range(n // 4):
            blk = om.chacha20_block(key, (i * n) // 4 + b, index)
            for r in range(4):
                out[i, 4 * b + r] = int.from_bytes(blk[16 * r:16 * r + 16], "little") % qi
    return out


def expand_batch(q, n, key, first_index, count):
    """[count, k, n]: ciphertext i expands with nonce (first_index + i) mod 2^64"""
    return np.stack([expand_a(q, n, key, (int(first_index) + i) & M64) for i in range(count)]) if count else np.zeros((0, len(q), n), dtype=np.uint64)


def noise(orc, noise_key, index):
    """[n] int8: e of ciphertext `index`"""
    return orc.encrypt_draws(noise_key, int(index) & M64)[1]


def delta_lift(orc, plain):
    """[k, n]: Delta m' of add_plain (what EncLift computes)"""
    zero = np.zeros((2, orc.k, orc.n), dtype=np.uint64)
    return orc.add_plain(zero, np.ascontiguousarray(plain, dtype=np.uint64))[0]


def centred(orc, e):
    """[k, n]: the residues of the small integers e"""
    return np.stack([np.array([int(v) % qi for v in e], dtype=np.uint64) for qi in orc.q])


def target_phase(orc, plain, noise_key, index):
    """Delta m' - e in every residue"""
    lift, e = delta_lift(orc, plain), noise(orc, noise_key, index)
    return np.stack([np.array([(int(l) - int(v)) % qi for l, v in zip(lift[i], e)], dtype=np.uint64) for i, qi in enumerate(orc.q)])


def encrypt(orc, sk, plain, a_key, noise_key, index):
    """(c0, a), both [k, n]: c0 fixed THROUGH the phase -- the phase of (0, a) is a s, so c0 = target - a s; checked by decrypting"""
    a = expand_a(orc.q, orc.n, a_key, index)
    zero = np.zeros((orc.k, orc.n), dtype=np.uint64)
    a_s = orc.decrypt_phase(sk, np.stack([zero, a]))
    want = target_phase(orc, plain, noise_key, index)
    c0 = np.stack([np.array([(int(w) - int(x)) % qi for w, x in zip(want[i], a_s[i])], dtype=np.uint64) for i, qi in enumerate(orc.q)])
    assert np.array_equal(orc.decrypt_phase(sk, np.stack([c0, a])), want)
    return c0, a
