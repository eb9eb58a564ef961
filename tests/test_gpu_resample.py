"""GPU: fhe_remap (resampling with public per-output weights) bit for bit against its op-by-op specification on the CPU oracle
(tests/resample_oracle.py) and on the GPU Evaluator, on every kernel path; the edges of the lazy sums; Evaluator.resize_plain against
two remap calls, the oracle and itself in both pass orders; row shards; launch chunks; refusals; and the streaming server end to end
(client.send_resize -> server.server_resize_plain -> client.receive_pixels), also beside the ct x ct circuit it replaces."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import resample_oracle as ro

pytestmark = pytest.mark.gpu

SMALL = dict(n=1024, q=[0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001], t=1 << 14)
# preset, switches, the fhe_remap_path the case must run (include/fhe_hip.h)
CONTEXTS = [("SMALL", {}, 0), ("P4096", {}, 4), ("P4096", {"FHE_DCT_FORCE_U64": "1"}, 0), ("P8192", {}, 1), ("SEAL23_4096", {}, 1), ("PM58", {}, 2)]
_cache = {}


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


def _pair(fhe, om, name, **switches):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    key = (name, tuple(sorted(switches.items())))
    if key not in _cache:
        p = SMALL if name == "SMALL" else dict(n=2048, q=_primes_58(2048, 2), t=1 << 14) if name == "PM58" else om.PRESETS[name]
        _cache[key] = (fhe.SEALContext(p["n"], p["q"], p["t"], switches=switches or None), om.Oracle(p["n"], p["q"], p["t"]))
    return _cache[key]


def _path(fhe, ctx):
    return fhe._lib.load().fhe_remap_path(ctx.h)


VALUES = np.array([0.5, -0.25, 0.0, 1.0 / 3.0, 1e-40, 1.7153, -3.0, 0.5, 0.0703125, -1.0 / 7.0])     # entries 2 and 4 encode to zero, 0 and 7 are one value


def _random_plan(count, n_src, T, seed):
    """taps and weight ids with unused slots, zero-encoding entries and runs of one id; every output keeps at least one live term"""
    rng = np.random.default_rng(seed)
    taps = rng.integers(0, n_src, size=(count, T)).astype(np.uint32)
    wids = rng.integers(0, len(VALUES), size=(count, T)).astype(np.uint32)
    wids[rng.random((count, T)) < 0.2] = ro.SKIP
    wids[:, T // 2] = np.where(np.isin(wids[:, T // 2], (2, 4, ro.SKIP)), 5, wids[:, T // 2])       # a live term everywhere
    wids[1, :3] = 3                                                  # a run of one id
    wids[2, :] = ro.SKIP
    wids[2, T - 1] = 1                                               # only the last slot is live
    wids[3, 0], wids[3, 1] = 2, 4                                    # zero-encoding weights in front
    taps[0, 0], taps[count - 1, T - 1] = 0, n_src - 1
    return taps, wids


def _gpu_stepwise(fhe, ctx, ev, src, taps, wids, values):
    """every output through the GPU Evaluator's multiply_plain / add, one operation at a time"""
    import torch
    enc, plains = fhe.FractionalEncoder(ctx), {}

    def plain(v):
        if v not in plains:
            p = enc.encode(v)
            plains[v] = (fhe.PreparedPlain(ctx, p) if np.any(p) else None)
        return plains[v]

    rows = [ro.remap_output(ev.add, lambda x, v: ev.multiply_plain(x, plain(v)), lambda v: plain(v) is None, lambda i: src[i:i + 1].clone(), taps[o], wids[o], values)
            for o in range(len(taps))]
    return torch.cat(rows)


def _picks(count, seed, want=8):
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.arange(1, count - 1), size=min(count - 2, want - 2), replace=False) if count > 2 else []
    return sorted({0, count - 1} | {int(i) for i in rest})


@pytest.mark.parametrize("size", [1, 2, 3])
@pytest.mark.parametrize("preset,switches,path", CONTEXTS)
def test_remap_matches_oracle_and_evaluator(fhe, oracle_mod, preset, switches, path, size):
    import torch
    ctx, orc = _pair(fhe, oracle_mod, preset, **switches)
    assert _path(fhe, ctx) == path
    ev = fhe.Evaluator(ctx)
    n_src, count, T = 11, 12, 6
    taps, wids = _random_plan(count, n_src, T, seed=40 + size)
    table = fhe.WeightTable(ctx, VALUES)
    assert table.count == len(VALUES) and table.distinct == 7
    src = ctx.random_ct(n_src, size=size, seed=fhe.SEED + 17 * size)
    before = src.clone()
    out = ev.remap(table, src, taps, wids)
    assert tuple(out.shape) == (count, size, ctx.k, ctx.n) and torch.equal(src, before)
    # ALL outputs, bit for bit, against the same composition on the GPU Evaluator
    assert torch.equal(out, _gpu_stepwise(fhe, ctx, ev, src, taps, wids, VALUES))
    # a seeded sample (first and last included) against the CPU oracle
    host, got, ops = fhe.to_host(src), fhe.to_host(out), ro.OracleOps(orc)
    picks = _picks(count, seed=size)
    assert len(picks) >= 8 and picks[0] == 0 and picks[-1] == count - 1
    for o in picks:
        assert np.array_equal(got[o], ops.output(host, taps[o], wids[o], VALUES)), o
    # src_is_ntt and out_is_ntt, each on and off: the slot form is exactly fhe_ntt_forward's
    ntt_src = ev.ntt_forward(src)
    assert torch.equal(ev.remap(table, ntt_src, taps, wids, src_is_ntt=True), out)
    slots = ev.remap(table, src, taps, wids, out_is_ntt=True)
    assert torch.equal(slots, ev.ntt_forward(out))
    assert torch.equal(ev.remap(table, ntt_src, taps, wids, src_is_ntt=True, out_is_ntt=True), slots)
    assert torch.equal(src, before)
    torch.cuda.synchronize()


@pytest.mark.parametrize("weights", ["distinct", "one"])
@pytest.mark.parametrize("preset,path", [("P8192", 1), ("SEAL23_4096", 1), ("PM58", 2)])
def test_lazy_sum_edge(fhe, oracle_mod, preset, path, weights):
    """the largest summands the accumulate kernel can meet: every residue q_i - 1 in coefficient form, and (src_is_ntt) every SLOT q_i - 1,
    under 64 taps with 64 distinct weights (64 products, folded every 8) and 64 taps of one weight (one sum, folded every 16)"""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, preset)
    assert _path(fhe, ctx) == path
    ev, ops = fhe.Evaluator(ctx), ro.OracleOps(orc)
    values = np.array([-(i + 1) / 64.0 for i in range(64)]) if weights == "distinct" else np.array([-1.0])
    table = fhe.WeightTable(ctx, values)
    assert table.distinct == len(values)
    rng = np.random.default_rng(8)
    taps = rng.integers(0, 4, size=(3, 64)).astype(np.uint32)
    wids = np.tile(np.arange(64, dtype=np.uint32) % len(values), (3, 1))
    top = fhe.to_device(np.broadcast_to((np.array(ctx.q, dtype=np.uint64) - 1)[None, None, :, None], (4, 2, ctx.k, ctx.n)), ctx.device)
    host = fhe.to_host(top)
    out = fhe.to_host(ev.remap(table, top, taps, wids))
    for o in (0, 2):
        assert np.array_equal(out[o], ops.output(host, taps[o], wids[o], values)), o
    got = ev.remap(table, top, taps, wids, src_is_ntt=True)
    coeff = fhe.to_host(ev.ntt_inverse(top))
    for o in (0, 2):
        assert np.array_equal(fhe.to_host(got)[o], ops.output(coeff, taps[o], wids[o], values)), o
    assert torch.equal(ev.remap(table, top, taps, wids, src_is_ntt=True, out_is_ntt=True), ev.ntt_forward(got))


@pytest.mark.parametrize("preset", ["SMALL", "SEAL23_4096"])
@pytest.mark.parametrize("kernel,dw,dh,antialias,bits", [("catmull_rom", 4, 9, False, None), ("lanczos3", 4, 4, True, None), ("triangle", 10, 3, False, 12)])
def test_resize_plain(fhe, oracle_mod, preset, kernel, dw, dh, antialias, bits):
    """Evaluator.resize_plain == its two remap calls == the oracle's two-pass composition on a sample; both pass orders give the same
    bits; the library's plan is the independent model's"""
    import torch
    ctx, orc = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    sw, sh, ch = 7, 6, 2
    src = ctx.random_ct(sh * sw * ch, seed=321)
    px, py = ro.axis_plan(sw, dw, kernel, antialias, "half_pixel", bits), ro.axis_plan(sh, dh, kernel, antialias, "half_pixel", bits)
    results = {}
    for order in ("hv", "vh"):
        plan = fhe.resize_plan(sw, sh, dw, dh, kernel, channels=ch, antialias=antialias, weight_bits=bits, order=order)
        assert plan["source_rows"] == (0, sh) and plan["order"] == order
        out = ev.resize_plain(plan, src)
        assert tuple(out.shape) == (dh * dw * ch, 2, ctx.k, ctx.n)
        a, b = plan["passes"]
        ta, tb = fhe.WeightTable(ctx, a["values"]), fhe.WeightTable(ctx, b["values"])
        two = ev.remap(tb, ev.remap(ta, src, a["taps"], a["wids"]), b["taps"], b["wids"])         # through coefficient form
        assert torch.equal(out, two), order
        results[order] = out
    assert torch.equal(results["hv"], results["vh"])
    assert torch.equal(ev.resize_plain(fhe.resize_plan(sw, sh, dw, dh, kernel, channels=ch, antialias=antialias, weight_bits=bits), src), results["hv"])
    host, got, ops = fhe.to_host(src), fhe.to_host(results["hv"]), ro.OracleOps(orc)
    rng = np.random.default_rng(dw * dh)
    picks = [(0, 0, 0), (dw - 1, dh - 1, ch - 1), (dw - 1, 0, 0), (0, dh - 1, 1)]
    while len(picks) < 8:
        cand = (int(rng.integers(dw)), int(rng.integers(dh)), int(rng.integers(ch)))
        if cand not in picks:
            picks.append(cand)
    for (x, y, c) in picks:
        want = ro.resize_output(ops, host, sw, ch, px, py, x, y, c, order="hv")
        assert np.array_equal(got[(y * dw + x) * ch + c], want), (x, y, c)


@pytest.mark.parametrize("kernel,antialias", [("catmull_rom", False), ("lanczos3", True)])
def test_row_shards_concatenate(fhe, oracle_mod, kernel, antialias):
    """shards of the destination rows, each on its own resident window (the source rows it reads), give the whole-image result"""
    import torch
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    ev = fhe.Evaluator(ctx)
    sw, sh, ch = 5, 11, 3
    for dw, dh in ((7, 5), (3, 16)):
        src = ctx.random_ct(sh, sw * ch, seed=1234)
        whole = ev.resize_plain(fhe.resize_plan(sw, sh, dw, dh, kernel, channels=ch, antialias=antialias), src.view(-1, 2, ctx.k, ctx.n))
        for cut in range(1, dh):
            parts = []
            for rows in ((0, cut), (cut, dh)):
                plan = fhe.resize_plan(sw, sh, dw, dh, kernel, channels=ch, antialias=antialias, rows=rows)
                first, cnt = plan["source_rows"]
                parts.append(ev.resize_plain(plan, src[first:first + cnt].contiguous().view(-1, 2, ctx.k, ctx.n)))
            assert torch.equal(torch.cat(parts), whole), (dw, dh, cut)


@pytest.mark.parametrize("preset", ["SMALL", "SEAL23_4096"])
def test_launch_chunks_and_empty_batch(fhe, oracle_mod, preset):
    """The (tap, id) table travels in chunks of min(4096, 32768 / T) outputs: 512 with 64 slots, 4096 with 8.  Outputs either side of the
    boundary equal their own single-output runs; an empty batch is a no-op"""
    import torch
    ctx, _ = _pair(fhe, oracle_mod, preset)
    ev = fhe.Evaluator(ctx)
    src = ctx.random_ct(16, seed=55)
    rng = np.random.default_rng(5)
    table = fhe.WeightTable(ctx, VALUES)
    for T, boundary in ((64, 512), (8, 4096)):
        if boundary == 4096 and preset != "SMALL":
            continue
        taps, wids = _random_plan(boundary + 3, 16, T, seed=T)
        out = ev.remap(table, src, taps, wids)
        for o in (0, boundary - 1, boundary, boundary + 2):
            assert torch.equal(out[o:o + 1], ev.remap(table, src, taps[o:o + 1], wids[o:o + 1])), (T, o)
        del out
    assert tuple(ev.remap(table, src, np.zeros((0, 9), dtype=np.uint32), np.zeros((0, 9), dtype=np.uint32)).shape) == (0, 2, ctx.k, ctx.n)
    L = fhe._lib
    out = ctx.empty(1)
    out.fill_(7)
    one = np.zeros((1, 2), dtype=np.uint32)
    L.call("fhe_remap", ctx.h, table.h, C.c_void_p(src.data_ptr()), 16, 2, 0, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), 2,
           C.c_void_p(out.data_ptr()), 0, 0, None, 0, None)                                     # count == 0: nothing is read or written
    torch.cuda.synchronize()
    assert bool((out == 7).all())


def test_library_refuses_bad_calls_and_leaves_out_untouched(fhe, oracle_mod):
    import torch
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    other, _ = _pair(fhe, oracle_mod, "SEAL23_4096")
    L = fhe._lib
    table = fhe.WeightTable(ctx, VALUES)
    foreign = fhe.WeightTable(other, VALUES)
    src, out = ctx.random_ct(4, seed=1), ctx.empty(2)
    taps = np.zeros((2, 3), dtype=np.uint32)
    wids = np.zeros((2, 3), dtype=np.uint32)
    scr = torch.empty(src.numel() * 8, dtype=torch.uint8, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(C.c_void_p)

    def go(**kw):
        return L.call("fhe_remap", ctx.h, kw.get("table", table).h, p(kw.get("src", src)), kw.get("n_src", 4), kw.get("size", 2), 0, hp(kw.get("taps", taps)),
                      hp(kw.get("wids", wids)), kw.get("T", 3), p(kw.get("out", out)), kw.get("out_is_ntt", 0), 2, p(kw.get("scratch", scr)),
                      kw.get("bytes", scr.numel()), None)
    go()
    torch.cuda.synchronize()
    good = out.clone()
    bad_taps = taps.copy()
    bad_taps[1, 2] = 4
    bad_wids = wids.copy()
    bad_wids[1, 2] = len(VALUES)
    skipped = wids.copy()
    skipped[1, :] = ro.SKIP                                           # an output with no slot in use
    zeros = wids.copy()
    zeros[1, :] = (2, 4, ro.SKIP)                                     # ... and one whose live slots all multiply by the zero plaintext
    dead_tap = bad_taps.copy()                                        # a tap out of range in a SKIPPED slot is not looked at
    dead_wids = wids.copy()
    dead_wids[1, 2] = ro.SKIP
    out.fill_(7)
    for kw in (dict(taps=bad_taps), dict(wids=bad_wids), dict(wids=skipped), dict(wids=zeros), dict(size=0), dict(T=0), dict(T=65), dict(table=foreign),
               dict(bytes=scr.numel() - 8), dict(out=src[1:3]), dict(n_src=0), dict(scratch=out), dict(wids=skipped, out_is_ntt=1)):
        with pytest.raises(fhe.FheError):
            go(**kw)
        torch.cuda.synchronize()
        if "out" not in kw:
            assert bool((out == 7).all()), kw
    go(taps=dead_tap, wids=dead_wids)
    go()
    torch.cuda.synchronize()
    assert torch.equal(out, good)
    for bad in ([1e300], [1.0, 1e300]):                               # a value the encoder cannot hold
        with pytest.raises(fhe.FheError):
            fhe.WeightTable(ctx, bad)
    empty = fhe.WeightTable(ctx, [0.0, 1e-40])                        # every entry encodes to zero: the table exists, no output can use it
    assert empty.distinct == 0 and empty.count == 2
    with pytest.raises(fhe.FheError):
        fhe.Evaluator(ctx).remap(empty, src, taps, wids)
    torch.cuda.synchronize()


def _stream_records(fhe, ctx, path, count):
    out = np.zeros((count, 2, ctx.k, ctx.n), dtype=np.uint64)
    with open(path, "rb") as f:
        for i in range(count):
            fhe.server.read_ciphertext_into(f, out[i])
        assert f.read(1) == b""
    return out


def test_server_resize_plain_end_to_end(fhe, oracle_mod, tmp_path):
    """client.send_resize of tests/golden/boazbarak.jpg's 48x48 pixels -> server.server_resize_plain to 32x32 -> client.receive_pixels: the
    decrypted output equals the float64 resample rounded to 8 bits; the stream holds exactly Evaluator.resize_plain's records; rows=
    shards fill the same file; seal/resample_check agrees"""
    import os
    from PIL import Image
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    rgb = np.asarray(Image.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boazbarak.jpg")).convert("RGB"), dtype=np.uint8)
    assert rgb.shape == (48, 48, 3)
    w = h = 48
    dw = dh = 32
    kg = fhe.KeyGenerator(ctx, seed=22)
    enc = fhe.FractionalEncoder(ctx)
    fin, fout, fsh = (str(tmp_path / x) for x in ("in.ct", "out.ct", "shards.ct"))
    assert fhe.client.send_resize(ctx, fhe.DeviceEncryptor(ctx, kg.public_key()), enc, rgb, fin) == (w, h)
    stats = {}
    assert fhe.server.server_resize_plain(ctx, fin, fout, w, h, dw, dh, "catmull_rom", rows_per_step=5, stats=stats) == dw * dh
    decoded = []
    pixels = fhe.client.receive_pixels(ctx, fhe.Decryptor(ctx, kg.secret_key()), enc, fout, dw, dh, decoded=decoded)
    px, py = ro.axis_plan(w, dw, "catmull_rom"), ro.axis_plan(h, dh, "catmull_rom")
    want = ro.resample_float(rgb, px, py)
    got = np.array(decoded).reshape(dh, dw, 3)
    err = np.max(np.abs(got - want))
    print("server_resize_plain 48x48 -> 32x32 catmull_rom: max |decoded - float resample| = %.3g; %r" % (err, stats))
    assert err < 1e-9
    eight = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    assert np.array_equal(eight(got), eight(want))
    assert pixels.shape == (dh, dw, 3)
    # the same records as one Evaluator.resize_plain call on the whole image
    src = fhe.to_device(_stream_records(fhe, ctx, fin, w * h * 3), ctx.device)
    direct = fhe.to_host(fhe.Evaluator(ctx).resize_plain(fhe.resize_plan(w, h, dw, dh, "catmull_rom", channels=3), src))
    assert np.array_equal(_stream_records(fhe, ctx, fout, dw * dh * 3), direct)
    # three shards into one file, out of order
    for rows in ((20, 32), (0, 7), (7, 20)):
        assert fhe.server.server_resize_plain(ctx, fin, fsh, w, h, dw, dh, "catmull_rom", rows_per_step=4, rows=rows) == (rows[1] - rows[0]) * dw
    assert open(fsh, "rb").read() == open(fout, "rb").read()
    # the facade program (seal::hip::resize_plain)
    exe = os.path.join(os.path.dirname(fhe.LIB_PATH), "seal", "resample_check")
    assert os.path.exists(exe), "build() makes seal/resample_check"
    fcpp = str(tmp_path / "cpp.ct")
    r = subprocess.run([exe, fin, fcpp, str(w), str(h), str(dw), str(dh), "catmull_rom", "half_pixel", "0", "0", str(ctx.n), str(ctx.t)] + [hex(x) for x in ctx.q],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(fcpp, "rb").read() == open(fout, "rb").read()
    words = direct.reshape(-1)
    digest = int(np.sum(words * (2 * np.arange(words.size, dtype=np.uint64) + 1), dtype=np.uint64))
    m = re.search(r"digest=([0-9a-f]{16})", r.stdout)
    assert m and int(m.group(1), 16) == digest, r.stdout


@pytest.mark.parametrize("w,h,dw,dh,bits,rows_per_step", [(3, 16, 4, 48, None, 1), (3, 16, 2, 80, None, 1), (2, 4, 3, 256, 4, 4), (3, 16, 4, 48, None, 5), (5, 9, 3, 4, 6, 1)])
def test_server_windows_when_weights_are_exactly_zero(fhe, oracle_mod, tmp_path, w, h, dw, dh, bits, rows_per_step):
    """An output that samples exactly on a source row (odd integer enlargements: 16 -> 48 row 4 at u = 1.0) or whose edge weights round to
    zero (weight_bits) reads fewer rows than its neighbours, so a band's own first source row can lie BEYOND the next band's: the resident
    window must still only move forwards.  The stream equals Evaluator.resize_plain on the whole image, record for record; so do shards."""
    ctx, _ = _pair(fhe, oracle_mod, "SMALL")
    ty, wy = ro.axis_plan(h, dh, "catmull_rom", False, "half_pixel", bits)
    if dh > h:
        assert np.any(wy[:, 0] == 0.0) and np.any(wy[:, 0] != 0.0)                              # the case is what it claims to be
    kg = fhe.KeyGenerator(ctx, seed=23)
    enc = fhe.FractionalEncoder(ctx)
    rgb = np.random.default_rng(w * h + dh).integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    fin, fout, fsh = (str(tmp_path / x) for x in ("in.ct", "out.ct", "shards.ct"))
    assert fhe.client.send_resize(ctx, fhe.DeviceEncryptor(ctx, kg.public_key()), enc, rgb, fin) == (w, h)
    assert fhe.server.server_resize_plain(ctx, fin, fout, w, h, dw, dh, "catmull_rom", weight_bits=bits, rows_per_step=rows_per_step) == dw * dh
    src = fhe.to_device(_stream_records(fhe, ctx, fin, w * h * 3), ctx.device)
    direct = fhe.to_host(fhe.Evaluator(ctx).resize_plain(fhe.resize_plan(w, h, dw, dh, "catmull_rom", channels=3, weight_bits=bits), src))
    assert np.array_equal(_stream_records(fhe, ctx, fout, dw * dh * 3), direct)
    cut = dh // 3 + 1
    for rows in ((cut, dh), (0, cut)):
        assert fhe.server.server_resize_plain(ctx, fin, fsh, w, h, dw, dh, "catmull_rom", weight_bits=bits, rows_per_step=rows_per_step, rows=rows) == (rows[1] - rows[0]) * dw
    assert open(fsh, "rb").read() == open(fout, "rb").read()
    decoded = []
    fhe.client.receive_pixels(ctx, fhe.Decryptor(ctx, kg.secret_key()), enc, fout, dw, dh, decoded=decoded)
    want = ro.resample_float(rgb, ro.axis_plan(w, dw, "catmull_rom", False, "half_pixel", bits), (ty, wy))
    assert np.max(np.abs(np.array(decoded).reshape(dh, dw, 3) - want)) < 1e-9


def test_reference_pair_decrypts_like_the_ct_x_ct_resize(fhe, oracle_mod, tmp_path):
    """REFERENCE_CUBIC weights with the REFERENCE coordinates are what ResizeImage / SampleBicubic compute with encrypted offsets
    (fhe_resize_bicubic_shared through server.server_resize): on the same encrypted image both streams decrypt to the same pixel values.
    The ciphertexts differ (two polynomials here, six there)."""
    ctx = fhe.SEALContext.preset("P8192")
    kg = fhe.KeyGenerator(ctx, seed=14)
    enc = fhe.FractionalEncoder(ctx)
    W, H, w, h = 6, 7, 4, 4
    rgb = np.random.default_rng(2).integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    fin, f_ct, f_plain = (str(tmp_path / x) for x in ("in.ct", "ctct.ct", "plain.ct"))
    assert fhe.client.send_resize(ctx, fhe.DeviceEncryptor(ctx, kg.public_key(), key=bytes(32)), enc, rgb, fin) == (W, H)
    fractions = fhe.server.make_fraction_encryptor(ctx, kg.public_key(), enc, seed=3, device=True)
    assert fhe.server.server_resize(ctx, fin, f_ct, W, H, w, h, True, fractions, rows_per_step=2, shared_offsets=True) == w * h
    assert fhe.server.server_resize_plain(ctx, fin, f_plain, W, H, w, h, "reference_cubic", convention="reference", rows_per_step=3) == w * h
    dec = fhe.Decryptor(ctx, kg.secret_key())
    a, b = [], []
    fhe.client.receive_resize(ctx, dec, enc, f_ct, w, h, decoded=a)
    fhe.client.receive_pixels(ctx, dec, enc, f_plain, w, h, decoded=b)
    a, b = np.array(a), np.array(b)
    assert a.shape == b.shape == (w * h * 3,)
    print("reference pair %dx%d -> %dx%d: max |ct x ct - plain weights| of the decoded doubles = %.3g" % (W, H, w, h, np.max(np.abs(a - b))))
    assert np.array_equal(np.rint(a).astype(np.int64), np.rint(b).astype(np.int64))
    # and both are the float resample with the reference's weights
    want = ro.resample_float(rgb, ro.axis_plan(W, w, "reference_cubic", False, "reference"), ro.axis_plan(H, h, "reference_cubic", False, "reference"))
    assert np.max(np.abs(b.reshape(h, w, 3) - want)) < 1e-9
