"""Specification of the sparse integer map across position-packed ciphertexts (include/fhe_hip.h: fhe_plane_map), twice: as the op-by-op
composition on the UNCHANGED CPU oracle (multiply_plain with a one-coefficient plaintext, add), and as a direct integer evaluation modulo
each q_i in numpy.  tests/test_planemap_cpu.py checks that the two agree; the GPU tests compare the library's bits with the direct form.
Nothing here calls the library."""
import numpy as np

import packed_oracle as po

EDGE_TERMS = (1, 8, 9, 16, 17, 64)      # live terms per output where the kernel's chunks of eight begin, end and are full


def plane_map_compose(orc, planes, taps, weights):
    """planes: [n_in][size, k, n]; output o = add over its slots p, in order, of multiply_plain(planes[taps[o][p]], [w mod t]), zero
    weights skipped"""
    return np.stack([po._weighted_sum(orc, [(w, planes[int(tp)] if int(w) else None) for tp, w in zip(trow, wrow)]) for trow, wrow in zip(taps, weights)])


def plane_map_direct(q, planes, taps, weights):
    """planes: uint64 [..., n_in, size, k, n] -> [..., n_out, size, k, n], residue by residue"""
    planes = np.asarray(planes, dtype=np.uint64)
    taps, weights = np.asarray(taps), np.asarray(weights)
    out = np.empty(planes.shape[:-4] + (taps.shape[0],) + planes.shape[-3:], dtype=np.uint64)
    for i, qi in enumerate(q):
        for o in range(taps.shape[0]):
            out[..., o, :, i, :] = po._lin([(w, planes[..., int(tp), :, i, :] if int(w) else None) for tp, w in zip(taps[o], weights[o])], qi)
    return out


def random_plan(rng, t, n_in, n_out, T, live_counts=()):
    """taps, weights [n_out][T] over the whole scalar range with zeros, repeated sources and both ends of the range; the first outputs
    get exactly live_counts live terms (the taps of a dead slot point past n_in: a skipped slot is not looked at); order: a shuffle"""
    lim = po.scalar_limit(t)
    taps = rng.integers(0, n_in, size=(n_out, T)).astype(np.uint32)
    w = rng.integers(-lim, lim + 1, size=(n_out, T), dtype=np.int64)
    w[w == 0] = 1
    dead = rng.random((n_out, T)) < 0.6
    for o in range(n_out):
        if o < len(live_counts):
            dead[o] = True
            dead[o, rng.permutation(T)[:live_counts[o]]] = False
        elif dead[o].all():
            dead[o, 0] = False
    w[dead] = 0
    taps[dead] = n_in + 7
    for o in range(n_out):
        live = np.nonzero(~dead[o])[0]
        w[o, live[0]] = lim if o % 2 else -lim
        if live.size > 1:
            taps[o, live[1]] = taps[o, live[0]]                        # the same source twice: two terms
            w[o, live[-1]] = -lim if o % 2 else lim
    return taps, w, rng.permutation(n_out).astype(np.uint32)
