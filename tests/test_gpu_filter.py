"""GPU: fhe_filter2d (2-D convolution with public weights) bit for bit against its op-by-op specification on the CPU oracle
(tests/filter_oracle.py) and on the GPU Evaluator, on every kernel path; the edges of the lazy sums; launch chunks; row shards;
and the streaming server end to end (client.send_resize -> server.server_filter -> client.receive_pixels, seal/filter_check)."""
import os
import re
import subprocess

import numpy as np
import pytest

import filter_oracle as fo

pytestmark = pytest.mark.gpu

SMALL = dict(n=1024, q=[0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001], t=1 << 14)
W, H = 6, 5
# preset, switches, the fhe_filter_path the case must run (include/fhe_hip.h)
CONTEXTS = [("SMALL", {}, 0), ("P4096", {}, 4), ("P8192", {}, 1), ("SEAL23_4096", {}, 1),
            ("P4096", {"FHE_DCT_FORCE_U64": "1"}, 0), ("P8192", {"FHE_NTT_NOPM": "1"}, 0)]
_cache = {}


def _pair(fhe, om, name, **switches):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    key = (name, tuple(sorted(switches.items())))
    if key not in _cache:
        p = dict(n=name[0], q=list(name[1]), t=name[2]) if isinstance(name, tuple) else SMALL if name == "SMALL" else om.PRESETS[name]
        _cache[key] = (fhe.SEALContext(p["n"], p["q"], p["t"], switches=switches or None), om.Oracle(p["n"], p["q"], p["t"]))
    return _cache[key]


def _path(fhe, ctx):
    return fhe._lib.load().fhe_filter_path(ctx.h)


def _sample_outputs(count, dst_w, dst_h, channels, seed, want=8):
    """the four corners (clamped taps) of channel 0 and seeded others, at least `want` outputs (all of them if there are fewer)"""
    corners = {(y * dst_w + x) * channels for y in (0, dst_h - 1) for x in (0, dst_w - 1)}
    rest = [i for i in range(count) if i not in corners]
    rng = np.random.default_rng(seed)
    extra = rng.choice(rest, size=min(len(rest), max(0, want - len(corners))), replace=False) if rest else []
    return sorted(corners | {int(i) for i in extra})


def _is_prime(m):
    if m % 2 == 0:
        return False
    d, s = m - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):          # deterministic below 3.3e24
        x = pow(a, d, m)
        if x in (1, m - 1):
            continue
        for _ in range(s - 1):
            x = x * x % m
            if x == m - 1:
                break
        else:
            return False
    return True


def _primes_58(n, count):
    """the largest `count` 58-bit primes = 1 (mod 2n): the pseudo-Mersenne class 2 of csrc/ntt_core.h (no preset has one as q-base)"""
    out, m = [], (1 << 58) + 1
    while len(out) < count:
        m -= 2 * n
        if _is_prime(m):
            out.append(m)
    return out


@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("kernel", ["box3", "sobel_x", "gauss5", "box7", "chroma420"])
@pytest.mark.parametrize("preset,switches,path", CONTEXTS)
def test_filter_matches_oracle(fhe, oracle_mod, preset, switches, path, kernel, size):
    ctx, orc = _pair(fhe, oracle_mod, preset, **switches)
    assert _path(fhe, ctx) == path
    weights, anchor, stride = fo.KERNELS[kernel]
    kh, kw = weights.shape
    taps = fo.tap_plan(W, H, 1, kw, kh, anchor, stride)
    dw, dh = fo.dst_size(W, H, stride)
    src = ctx.random_ct(W * H, size=size, seed=fhe.SEED + 31 * size)
    out = fhe.to_host(fhe.Evaluator(ctx).filter2d(fhe.FilterPlan(ctx, weights), src, taps))
    host = fhe.to_host(src)
    ops = fo.OracleOps(orc)
    picks = _sample_outputs(len(taps), dw, dh, 1, seed=len(kernel) + size)
    assert len(picks) >= 8 and {0, dw - 1, (dh - 1) * dw, dh * dw - 1} <= set(picks)
    for o in picks:
        assert np.array_equal(out[o], ops.output(host, taps[o], weights)), (kernel, o)


def test_filter_on_pseudo_mersenne_class_2(fhe, oracle_mod):
    """58-bit primes: k_tap_sum_pm on class PmB (products below 1.5 q), including the all-(q - 1) sums"""
    import torch
    n = 2048
    ctx, orc = _pair(fhe, oracle_mod, (n, tuple(_primes_58(n, 2)), 1 << 14))
    assert _path(fhe, ctx) == 2
    ev, ops = fhe.Evaluator(ctx), fo.OracleOps(orc)
    for kernel in ("gauss5", "box7", "minus8x8"):
        weights, anchor, stride = fo.KERNELS[kernel]
        taps = fo.tap_plan(W, H, 1, weights.shape[1], weights.shape[0], anchor, stride)
        src = ctx.random_ct(W * H, seed=77)
        out = fhe.to_host(ev.filter2d(fhe.FilterPlan(ctx, weights), src, taps))
        host = fhe.to_host(src)
        for o in (0, 14, len(taps) - 1):
            assert np.array_equal(out[o], ops.output(host, taps[o], weights)), (kernel, o)
        top = fhe.to_device(np.broadcast_to((np.array(ctx.q, dtype=np.uint64) - 1)[None, None, :, None], (W * H, 2, ctx.k, n)), ctx.device)
        out = fhe.to_host(ev.filter2d(fhe.FilterPlan(ctx, weights), top, taps, src_is_ntt=True))
        coeff = fhe.to_host(ev.ntt_inverse(top))
        assert np.array_equal(out[7], ops.output(coeff, taps[7], weights)), kernel
    torch.cuda.synchronize()


def test_plain_workgroup_order_gives_the_same_bits(fhe, oracle_mod):
    """FHE_FILTER_XCD=0 (the shared-ids rows in plain workgroup order, the launch arm only this switch reaches) against the default
    order, at a grid that is no multiple of the eight XCDs: idle workgroups and outputs that straddle XCD runs"""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, "SEAL23_4096")
    plain, _ = _pair(fhe, oracle_mod, "SEAL23_4096", FHE_FILTER_XCD="0")
    assert _path(fhe, ctx) == 1 and _path(fhe, plain) == 1
    weights, anchor, stride = fo.KERNELS["gauss3"]
    size = 3
    taps = fo.tap_plan(3, 3, 1, 3, 3, anchor, stride)
    assert len(taps) * size * ctx.k == 54 and 54 % 8 != 0
    src = ctx.random_ct(9, size=size, seed=fhe.SEED + 54)
    out = fhe.Evaluator(ctx).filter2d(fhe.FilterPlan(ctx, weights), src, taps)
    assert torch.equal(out, fhe.Evaluator(plain).filter2d(fhe.FilterPlan(plain, weights), src, taps))
    assert np.array_equal(fhe.to_host(out)[4], fo.OracleOps(orc).output(fhe.to_host(src), taps[4], weights))


@pytest.mark.parametrize("kernel", ["sobel_x", "gauss5", "chroma420"])
@pytest.mark.parametrize("preset,path", [("SMALL", 0), ("SEAL23_4096", 1), ("PM58", 2)])
def test_filter2d_equals_remap(fhe, oracle_mod, preset, path, kernel):
    """the identity the shared kernels rest on: fhe_filter2d is fhe_remap with every output naming the kernel positions 0 .. kw * kh - 1
    as its weight ids (zero weights: skipped slots; equal weights: runs in the filter, single taps in the remap); both are exact"""
    import torch
    name = (2048, tuple(_primes_58(2048, 2)), 1 << 14) if preset == "PM58" else preset
    ctx, _ = _pair(fhe, oracle_mod, name)
    assert _path(fhe, ctx) == path and fhe._lib.load().fhe_remap_path(ctx.h) == path
    ev = fhe.Evaluator(ctx)
    weights, anchor, stride = fo.KERNELS[kernel]
    kh, kw = weights.shape
    taps = fo.tap_plan(W, H, 1, kw, kh, anchor, stride)
    src = ctx.random_ct(W * H, size=2, seed=fhe.SEED + 7)
    wids = np.broadcast_to(np.arange(kw * kh, dtype=np.uint32), (len(taps), kw * kh))
    filtered = ev.filter2d(fhe.FilterPlan(ctx, weights), src, taps)
    assert torch.equal(filtered, ev.remap(fhe.WeightTable(ctx, weights.ravel()), src, taps, wids))


@pytest.mark.parametrize("kernel", ["box7", "minus8x8"])
@pytest.mark.parametrize("preset,switches,path", [c for c in CONTEXTS if c[0] != "SMALL"])
def test_lazy_sum_edge(fhe, oracle_mod, preset, switches, path, kernel):
    """the largest summands the accumulate kernel can meet: every residue q_i - 1 in coefficient form, and (src_is_ntt) every SLOT
    q_i - 1, under 49 and 64 equal weights (one lazy sum over all taps, folded every 16 summands)"""
    ctx, orc = _pair(fhe, oracle_mod, preset, **switches)
    assert _path(fhe, ctx) == path
    ev, ops = fhe.Evaluator(ctx), fo.OracleOps(orc)
    weights, anchor, stride = fo.KERNELS[kernel]
    taps = fo.tap_plan(4, 4, 1, weights.shape[1], weights.shape[0], anchor, stride)
    plan = fhe.FilterPlan(ctx, weights)
    assert plan.taps == weights.size
    top = fhe.to_device(np.broadcast_to((np.array(ctx.q, dtype=np.uint64) - 1)[None, None, :, None], (16, 2, ctx.k, ctx.n)), ctx.device)
    host = fhe.to_host(top)
    out = fhe.to_host(ev.filter2d(plan, top, taps))
    for o in (0, 5):
        assert np.array_equal(out[o], ops.output(host, taps[o], weights)), o
    out = fhe.to_host(ev.filter2d(plan, top, taps, src_is_ntt=True))
    coeff = fhe.to_host(ev.ntt_inverse(top))
    for o in (0, 5):
        assert np.array_equal(out[o], ops.output(coeff, taps[o], weights)), o


@pytest.mark.parametrize("kernel", ["gauss3", "sobel_x", "chroma420"])
def test_filter_equals_evaluator_calls_and_leaves_src(fhe, oracle_mod, kernel):
    """whole image, three channels, on SMALL: one multiply_plain / add at a time on the GPU Evaluator gives the same bits; so does the
    call on ntt_forward(src) with src_is_ntt; src is not written"""
    import torch
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    ev, enc = fhe.Evaluator(ctx), fhe.FractionalEncoder(ctx)
    weights, anchor, stride = fo.KERNELS[kernel]
    kh, kw = weights.shape
    taps = fo.tap_plan(W, H, 3, kw, kh, anchor, stride)
    src = ctx.random_ct(W * H * 3, seed=909)
    before = src.clone()
    plan = fhe.FilterPlan(ctx, weights)
    fused = ev.filter2d(plan, src, taps)
    assert torch.equal(src, before)
    idx = torch.as_tensor(taps, device=ctx.device)

    def M(x, v):
        return ev.multiply_plain(x, fhe.PreparedPlain(ctx, enc.encode(v)))

    stepwise = fo.filter_output(ev.add, M, lambda v: not np.any(enc.encode(v)), lambda p: src[idx[:, p]].contiguous(), list(range(kw * kh)), weights)
    assert torch.equal(fused, stepwise)
    assert torch.equal(ev.filter2d(plan, ev.ntt_forward(src), taps, src_is_ntt=True), fused)
    assert torch.equal(src, before)
    # the library's own tap plan is the independent model's
    mine, dw, dh = fhe.filter_tap_plan(W, H, kw, kh, channels=3, anchor=anchor, stride=stride)
    assert (dw, dh) == fo.dst_size(W, H, stride) and np.array_equal(mine, taps)


@pytest.mark.parametrize("kernel", ["gauss5", "chroma420"])
def test_row_shards_concatenate(fhe, oracle_mod, kernel):
    """two shards of the destination rows, each on its own resident window (its rows + the halo), give the whole-image result"""
    import torch
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    weights, anchor, stride = fo.KERNELS[kernel]
    kh, kw = weights.shape
    w, h = 5, 9
    src = ctx.random_ct(h, w * 3, seed=1234)
    plan = fhe.FilterPlan(ctx, weights)
    taps, dw, dh = fhe.filter_tap_plan(w, h, kw, kh, channels=3, anchor=anchor, stride=stride)
    whole = ev.filter2d(plan, src.view(-1, 2, ctx.k, ctx.n), taps)
    for cut in range(1, dh):
        parts = []
        for rows in ((0, cut), (cut, dh)):
            first, cnt = fhe.filter_source_rows(h, kh, anchor[1], stride[1], *rows)
            t, _, _ = fhe.filter_tap_plan(w, h, kw, kh, channels=3, anchor=anchor, stride=stride, rows=rows, src_row0=first)
            window = src[first:first + cnt].contiguous().view(-1, 2, ctx.k, ctx.n)
            parts.append(ev.filter2d(plan, window, t))
        assert torch.equal(torch.cat(parts), whole), cut


@pytest.mark.parametrize("preset,switches", [("SMALL", {}), ("SEAL23_4096", {})])
def test_launch_chunks_and_empty_batch(fhe, oracle_mod, preset, switches):
    """The tap table travels in chunks of min(4096, 65536 / taps) outputs: 1024 with 64 taps, 4096 with 9.  Outputs either side of the
    boundary equal their own single-output runs; an empty batch is a no-op"""
    import torch
    ctx, _ = _pair(fhe, oracle_mod, preset, **switches)
    ev = fhe.Evaluator(ctx)
    src = ctx.random_ct(16, seed=55)
    rng = np.random.default_rng(5)
    for kernel, boundary in (("minus8x8", 1024), ("box3", 4096)):
        if boundary == 4096 and preset != "SMALL":
            continue
        weights = fo.KERNELS[kernel][0]
        plan = fhe.FilterPlan(ctx, weights)
        taps = rng.integers(0, 16, size=(boundary + 3, weights.size))
        out = ev.filter2d(plan, src, taps)
        for o in (0, boundary - 1, boundary, boundary + 2):
            assert torch.equal(out[o:o + 1], ev.filter2d(plan, src, taps[o:o + 1])), (kernel, o)
        del out
    plan = fhe.FilterPlan(ctx, fo.KERNELS["box3"][0])
    assert tuple(ev.filter2d(plan, src, np.zeros((0, 9), dtype=np.uint32)).shape) == (0, 2, ctx.k, ctx.n)
    torch.cuda.synchronize()


def test_library_refuses_bad_calls(fhe, oracle_mod):
    import ctypes as C
    import torch
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    other, _ = _pair(fhe, oracle_mod, "SEAL23_4096")
    L = fhe._lib
    plan = fhe.FilterPlan(ctx, fo.KERNELS["box3"][0])
    src, out = ctx.random_ct(4, seed=1), ctx.empty(2)
    taps = np.zeros((2, 9), dtype=np.uint32)
    scr = torch.empty(src.numel() * 8, dtype=torch.uint8, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    tp = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = lambda **kw: L.call("fhe_filter2d", kw.get("ctx", ctx.h), plan.h, p(kw.get("src", src)), kw.get("n_src", 4), kw.get("size", 2), 0, tp(kw.get("taps", taps)),
                             p(kw.get("out", out)), 2, p(scr), kw.get("bytes", scr.numel()), None)
    ok()
    bad_taps = taps.copy()
    bad_taps[1, 8] = 4
    for kw in (dict(taps=bad_taps), dict(size=0), dict(ctx=other.h), dict(bytes=scr.numel() - 8), dict(out=src[1:3]), dict(n_src=0)):
        with pytest.raises(fhe.FheError):
            ok(**kw)
    with pytest.raises(fhe.FheError):
        fhe.FilterPlan(ctx, [[1e-40]])                         # encodes to the zero plaintext: every weight zero for the library
    torch.cuda.synchronize()


def _stream_records(fhe, ctx, path, count):
    out = np.zeros((count, 2, ctx.k, ctx.n), dtype=np.uint64)
    with open(path, "rb") as f:
        for i in range(count):
            fhe.server.read_ciphertext_into(f, out[i])
        assert f.read(1) == b""
    return out


@pytest.mark.parametrize("kernel", ["gauss3", "chroma420"])
def test_server_filter_end_to_end(fhe, oracle_mod, tmp_path, kernel):
    """client.send_resize of a 12x10 RGB image -> server.server_filter -> client.receive_pixels decrypts to the float convolution; the
    output stream holds exactly Evaluator.filter2d's records; two rows= shards fill the same file; seal/filter_check agrees"""
    ctx, _ = _pair(fhe, oracle_mod, "P4096")
    w, h = 12, 10
    weights, anchor, stride = fo.KERNELS[kernel]
    kh, kw = weights.shape
    kg = fhe.KeyGenerator(ctx, seed=21)
    enc = fhe.FractionalEncoder(ctx)
    rgb = np.random.default_rng(1210).integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    fin, fout, fsh, fcpp = (str(tmp_path / x) for x in ("in.ct", "out.ct", "shards.ct", "cpp.ct"))
    assert fhe.client.send_resize(ctx, fhe.DeviceEncryptor(ctx, kg.public_key()), enc, rgb, fin) == (w, h)
    dw, dh = fo.dst_size(w, h, stride)
    assert fhe.server.server_filter(ctx, fin, fout, w, h, weights, anchor=anchor, stride=stride, rows_per_step=3) == dw * dh
    decoded = []
    fhe.client.receive_pixels(ctx, fhe.Decryptor(ctx, kg.secret_key()), enc, fout, dw, dh, decoded=decoded)
    want = fo.conv_float(rgb, weights, anchor, stride)
    err = np.max(np.abs(np.array(decoded).reshape(dh, dw, 3) - want))
    print("server_filter %s: max |decoded - float convolution| = %.3g" % (kernel, err))
    assert err < 1e-6
    # the same records as one Evaluator.filter2d call on the whole image
    src = fhe.to_device(_stream_records(fhe, ctx, fin, w * h * 3), ctx.device)
    taps = fo.tap_plan(w, h, 3, kw, kh, anchor, stride)
    direct = fhe.to_host(fhe.Evaluator(ctx).filter2d(fhe.FilterPlan(ctx, weights), src, taps))
    assert np.array_equal(_stream_records(fhe, ctx, fout, dw * dh * 3), direct)
    # two shards into one file
    cut = dh // 2
    for rows in ((cut, dh), (0, cut)):
        assert fhe.server.server_filter(ctx, fin, fsh, w, h, weights, anchor=anchor, stride=stride, rows_per_step=2, rows=rows) == (rows[1] - rows[0]) * dw
    assert open(fsh, "rb").read() == open(fout, "rb").read()
    # the facade program
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "filter_check")
    assert os.path.exists(exe), "build() makes seal/filter_check"
    r = subprocess.run([exe, fin, fcpp, str(w), str(h), kernel, str(ctx.n), str(ctx.t)] + [hex(x) for x in ctx.q], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(fcpp, "rb").read() == open(fout, "rb").read()
    words = direct.reshape(-1)
    digest = int(np.sum(words * (2 * np.arange(words.size, dtype=np.uint64) + 1), dtype=np.uint64))
    m = re.search(r"digest=([0-9a-f]{16})", r.stdout)
    assert m and int(m.group(1), 16) == digest, r.stdout
