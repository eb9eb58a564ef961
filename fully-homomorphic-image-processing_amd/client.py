"""Client side of the JPEG pipeline: the two halves of homo/client_jpeg.cpp over this package's
KeyGenerator / Encryptor / Decryptor.  Plaintext, CPU-side work.

  send_jpeg     -- homo/client_jpeg.cpp:73-166: every pixel encoded (FractionalEncoder) and encrypted,
                   written as 8x8 blocks: 64 R, 64 G, 64 B ciphertexts per block, blocks row-major
                   (split_image_eight_block, homo/fhe_image.h:108-124)
  receive_jpeg  -- homo/client_jpeg.cpp:196-296: per block and channel decrypt + decode 64 coefficients,
                   round half away from zero (:277), place in zig-zag order, entropy-code the block
                   (DC difference + run-length AC symbols, the baseline Huffman tables of ITU-T T.81
                   Annex K) into a JFIF file with all-ones quantisation tables (QUALITY = 0,
                   homo/fhe_image.h:32) and 1x1 sampling for Y, Cb, Cr
  rms_error     -- the quantity of compare_jpeg_jojpeg (homo/fhe_image.h:508-521) between two decoded images

The Huffman code tables are derived here from the (counts per length, symbol values) specification of
Annex K (tables K.3-K.6) by the canonical-code construction of T.81 Annex C, not transcribed."""
import math
import os

import numpy as np

from . import server

# zig-zag position of natural-order coefficient i (T.81 Figure 5)
ZIGZAG = np.zeros(64, dtype=np.int64)
_order, _i, _j = [], 0, 0
for _s in range(15):
    _rng = range(max(0, _s - 7), min(_s, 7) + 1)
    for _r in (_rng if _s % 2 else reversed(_rng)):
        _order.append(_r * 8 + (_s - _r))
for _pos, _nat in enumerate(_order):
    ZIGZAG[_nat] = _pos

# T.81 Annex K.3: number of codes of each length 1..16 and the symbol values, in order
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
    0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
    0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
    0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
    0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
    0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA])


def _canonical_codes(spec):
    """T.81 Annex C: symbol -> (code, length) from (counts per length, values)."""
    counts, values = spec
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


class _BitWriter:
    def __init__(self, f):
        self.f, self.acc, self.cnt = f, 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.cnt += length
        while self.cnt >= 8:
            byte = (self.acc >> (self.cnt - 8)) & 0xFF
            self.f.write(bytes([byte, 0]) if byte == 0xFF else bytes([byte]))      # byte stuffing after 0xFF
            self.cnt -= 8
        self.acc &= (1 << self.cnt) - 1


def _magnitude(v):
    """(additional bits, category): category = bit length of |v|, negative values as v - 1 (T.81 F.1.2.1)"""
    size = int(abs(v)).bit_length()
    return (v if v >= 0 else v - 1) & ((1 << size) - 1), size


def _encode_block(bw, du, dc_pred, htdc, htac):
    """one 8x8 block of zig-zag-ordered integer coefficients; returns the new DC predictor"""
    diff = du[0] - dc_pred
    if diff == 0:
        bw.put(*htdc[0])
    else:
        bits, size = _magnitude(diff)
        bw.put(*htdc[size])
        bw.put(bits, size)
    last = 63
    while last > 0 and du[last] == 0:
        last -= 1
    if last == 0:
        bw.put(*htac[0x00])                                  # end of block
        return du[0]
    i = 1
    while i <= last:
        run = 0
        while du[i] == 0 and i <= last:
            run += 1
            i += 1
        while run >= 16:
            bw.put(*htac[0xF0])                              # sixteen zeros
            run -= 16
        bits, size = _magnitude(du[i])
        bw.put(*htac[(run << 4) + size])
        bw.put(bits, size)
        i += 1
    if last != 63:
        bw.put(*htac[0x00])
    return du[0]


def _dht_segment(tc_th, spec):
    return bytes([tc_th]) + bytes(spec[0]) + bytes(spec[1])


def write_jpeg_from_coefficients(path, coeff_blocks, width, height):
    """coeff_blocks: iterable of [3][64] integer arrays (Y, Cb, Cr per 8x8 block, NATURAL order, already rounded),
    blocks row-major.  Writes a baseline JFIF file the way homo/client_jpeg.cpp:218-292 does: quantisation tables
    of ones, 1x1 sampling, the Annex K Huffman tables, one interleaved scan."""
    tables = [_canonical_codes(s) for s in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)]
    with open(path, "wb") as f:
        f.write(bytes([0xFF, 0xD8, 0xFF, 0xE0, 0, 0x10]) + b"JFIF\x00" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
        f.write(bytes([0xFF, 0xDB, 0, 0x84, 0]) + bytes([1] * 64) + bytes([1]) + bytes([1] * 64))
        f.write(bytes([0xFF, 0xC0, 0, 0x11, 8, height >> 8, height & 0xFF, width >> 8, width & 0xFF, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
        f.write(bytes([0xFF, 0xC4, 0x01, 0xA2]) + _dht_segment(0x00, DC_LUMA) + _dht_segment(0x10, AC_LUMA)
                + _dht_segment(0x01, DC_CHROMA) + _dht_segment(0x11, AC_CHROMA))
        f.write(bytes([0xFF, 0xDA, 0, 0xC, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 0x3F, 0]))
        bw = _BitWriter(f)
        pred = [0, 0, 0]
        for blk in coeff_blocks:
            for ch in range(3):
                zz = [0] * 64
                for j in range(64):
                    zz[int(ZIGZAG[j])] = int(blk[ch][j])
                ht = (tables[0], tables[1]) if ch == 0 else (tables[2], tables[3])
                pred[ch] = _encode_block(bw, zz, pred[ch], ht[0], ht[1])
        bw.put(0x7F, 7)                                       # pad the last byte with ones
        f.write(bytes([0xFF, 0xD9]))


def round_half_away(v):
    """homo/client_jpeg.cpp:277: v < 0 ? ceilf(v - 0.5f) : floorf(v + 0.5f), in float32 like the reference"""
    f = np.float32(v)
    return int(np.ceil(f - np.float32(0.5))) if v < 0 else int(np.floor(f + np.float32(0.5)))


def blocks_of(channel, width, height):
    """split_image_eight_block (homo/fhe_image.h:108-124): 8x8 blocks row-major, 64 values each"""
    a = np.asarray(channel).reshape(height, width)
    return [a[j:j + 8, i:i + 8].reshape(64) for j in range(0, height - height % 8, 8) for i in range(0, width - width % 8, 8)]


def send_jpeg(ctx, encryptor, encoder, rgb, out_path):
    """rgb: uint8 [H, W, 3].  Writes the ciphertext stream server.server_jpeg reads; returns the block count."""
    import torch
    h, w, _ = rgb.shape
    chans = [blocks_of(rgb[:, :, c].astype(np.float64), w, h) for c in range(3)]
    first = _seed_start(encryptor)
    with open(out_path, "wb") as f:
        _encrypt_values(ctx, encryptor, encoder, [v for b in range(len(chans[0])) for c in range(3) for v in chans[c][b]], f)
    _seed_finish(encryptor, first, out_path)
    return len(chans[0])


def receive_jpeg(ctx, decryptor, encoder, in_path, width, height, out_path):
    """Decrypt the server's stream (per block: 64 Y, 64 Cb, 64 Cr) and write the JPEG.  Returns the rounded
    coefficient blocks [n_blocks][3][64]."""
    n_blocks = (width // 8) * (height // 8)
    blocks = []
    with open(in_path, "rb") as f:
        for _ in range(n_blocks):
            recs = []
            for _ in range(192):
                ct = np.zeros((2, ctx.k, ctx.n), dtype=np.uint64)
                server.read_ciphertext_into(f, ct)
                recs.append(ct)
            plains = _decrypt_records(ctx, decryptor, recs)                 # one block's 64 Y, 64 Cb, 64 Cr in one fhe_decrypt_batch
            blk = np.zeros((3, 64), dtype=np.int64)
            for ch in range(3):
                for j in range(64):
                    blk[ch, j] = round_half_away(encoder.decode(plains[ch * 64 + j]))
            blocks.append(blk)
    write_jpeg_from_coefficients(out_path, blocks, width, height)
    return blocks


def rms_error(a, b):
    """compare_jpeg_jojpeg's number (homo/fhe_image.h:513-520) for two decoded uint8 images of equal shape"""
    d = np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)
    return math.sqrt(float((d * d).sum()) / d.size)


# ------------------------------------------------------------------------------------------------
# client halves of the resize and decode pipelines (homo/client_resize.cpp, homo/client_decode.cpp)
# ------------------------------------------------------------------------------------------------
def _encrypt_values(ctx, encryptor, encoder, values, f, chunk=1024):
    """encode + encrypt + write, in stream order.  A keys.DeviceEncryptor (anything with `encrypt_values`) works in device batches
    (fhe_frac_encode_batch + fhe_encrypt_batch, one download per chunk); a keys.Encryptor one ciphertext at a time.  A
    keys.SymmetricEncryptor (`seeded`) writes records of ONE polynomial, c0; the callers write the seed beside the stream (write_seed)."""
    import torch
    if hasattr(encryptor, "encrypt_values"):
        if (encryptor.int_coeffs, encryptor.frac_coeffs) != (encoder.int_coeffs, encoder.frac_coeffs):
            raise ValueError("the encryptor's encoder parameters differ from the encoder's")
        values = [float(v) for v in values]
        for s in range(0, len(values), chunk):
            cts = encryptor.encrypt_values(values[s:s + chunk])
            if getattr(encryptor, "seeded", False):
                cts = cts.c0[:, None]                            # [count, 1, k, n]: the existing record format with polys = 1
            torch.cuda.synchronize()
            for ct in cts.cpu().numpy().view(np.uint64):
                server.write_ciphertext(f, ct)
        return
    for v in values:
        ct = encryptor.encrypt(encoder.encode(float(v)))
        torch.cuda.synchronize()
        server.write_ciphertext(f, ct.cpu().numpy().view(np.uint64))


# ---- seeded streams (keys.SymmetricEncryptor): records of c0 alone, and 40 bytes beside them -------------------------
SEED_SUFFIX = ".seed"
SEED_BYTES = 40


def write_seed(path, a_key, first_index):
    """the sidecar of a seeded stream: the public a_key (32 bytes), then the number of the stream's first ciphertext as a little-endian
    u64 -- record r expands with index first_index + r (Evaluator.expand_seeded, server_jpeg(seeded="sidecar"))"""
    a_key = bytes(a_key)
    if len(a_key) != 32:
        raise ValueError("a_key has 32 bytes")
    with open(path, "wb") as f:
        f.write(a_key + (int(first_index) & ((1 << 64) - 1)).to_bytes(8, "little"))


def read_seed(path):
    """(a_key, first_index) of write_seed; a file of any other length is refused"""
    with open(path, "rb") as f:
        raw = f.read(SEED_BYTES + 1)
    if len(raw) != SEED_BYTES:
        raise ValueError("%s: a seed file has %d bytes (a_key, first_index)" % (path, SEED_BYTES))
    return raw[:32], int.from_bytes(raw[32:], "little")


def _seed_start(encryptor):
    return encryptor.next if getattr(encryptor, "seeded", False) else None


def _seed_finish(encryptor, first, out_path):
    if first is not None:
        write_seed(os.fspath(out_path) + SEED_SUFFIX, encryptor.a_key, first)


def send_resize(ctx, encryptor, encoder, rgb, out_path):
    """homo/client_resize.cpp:141-158: every sample of the image encoded and encrypted, "RGBRGB... row by row" (:141),
    the stream server.server_resize reads.  rgb: uint8 [H, W, 3].  Returns (width, height)."""
    h, w, _ = rgb.shape
    first = _seed_start(encryptor)
    with open(out_path, "wb") as f:
        _encrypt_values(ctx, encryptor, encoder, np.asarray(rgb, dtype=np.uint8).reshape(-1), f)
    _seed_finish(encryptor, first, out_path)
    return w, h


def to_pixel(value, clamp=True):
    """`int pixel = encoder.decode(p); CLAMP(pixel, 0, 255); (uint8_t) pixel` (homo/client_resize.cpp:206-209,
    homo/client_decode.cpp:205-207): truncation toward zero, saturated to int as x86 cvttsd2si does for values
    outside the int range (INT_MIN), then the clamp.  clamp=False is the same conversion without the CLAMP line --
    the client that produced the bicubic t = 11 entries of benchmark/results.txt."""
    v = float(value)
    pixel = int(v) if math.isfinite(v) and abs(v) < 2147483648.0 else -2147483648
    if clamp:
        pixel = 0 if pixel < 0 else 255 if pixel > 255 else pixel
    return pixel & 0xFF


def _decrypt_records(ctx, decryptor, recs):
    """recs: host arrays [size, k, n] (sizes may differ: a decode stream interleaves 22- and 2-polynomial records) -> plaintexts in the
    same order; records of one size go through keys.Decryptor.decrypt_batch (fhe_decrypt_batch) together"""
    import torch
    plains = [None] * len(recs)
    if not hasattr(decryptor, "decrypt_batch"):
        return [decryptor.decrypt(torch.from_numpy(r.view(np.int64).copy()).to(ctx.device)) for r in recs]
    for size in sorted({r.shape[0] for r in recs}):
        idx = [i for i, r in enumerate(recs) if r.shape[0] == size]
        batch = torch.from_numpy(np.stack([recs[i] for i in idx]).view(np.int64)).to(ctx.device)
        for i, p in zip(idx, decryptor.decrypt_batch(batch)):
            plains[i] = p
    return plains


def receive_pixels(ctx, decryptor, encoder, in_path, width, height, clamp=True, decoded=None):
    """The receiving half shared by homo/client_resize.cpp:197-211 and homo/client_decode.cpp:200-209: width * height * 3
    records (ciphertexts of any size: 4 or 6 polynomials after a resize, 22 after the run-length decoder), each
    decrypted, decoded and converted by to_pixel.  Returns uint8 [height, width, 3]; `decoded` (a list) receives the
    decoded doubles in stream order."""
    out = np.zeros(width * height * 3, dtype=np.uint8)
    with open(in_path, "rb") as f:
        for first in range(0, out.size, 256):
            recs = []
            for i in range(first, min(first + 256, out.size)):
                hdr = f.read(server.RECORD_HEADER)
                if len(hdr) != server.RECORD_HEADER:
                    raise EOFError("ciphertext stream ended")
                magic, size, k, n, _ = server.HEADER.unpack(hdr)
                if magic != server.MAGIC or (k, n) != (ctx.k, ctx.n) or not 1 <= size <= 64:
                    raise ValueError("not a ciphertext record of this context")
                ct = np.frombuffer(f.read(size * k * n * 8), dtype=np.uint64)
                if ct.size != size * k * n:
                    raise EOFError("truncated ciphertext record")
                recs.append(ct.reshape(size, k, n))
            for i, plain in enumerate(_decrypt_records(ctx, decryptor, recs)):
                v = encoder.decode(plain)
                if decoded is not None:
                    decoded.append(v)
                out[first + i] = to_pixel(v, clamp)
    return out.reshape(height, width, 3)


def receive_resize(ctx, decryptor, encoder, in_path, width, height, clamp=True, decoded=None):
    """homo/client_resize.cpp:163-222 without its OpenCV comparison: the resized image, uint8 [height, width, 3]"""
    return receive_pixels(ctx, decryptor, encoder, in_path, width, height, clamp, decoded)


def run_length_pairs(channel):
    """The run-length encoder of homo/client_decode.cpp:126-148 for one colour channel (values in scan order):
    [(value, count), ...]"""
    vals = [int(v) for v in channel]
    runs, curr, count = [], vals[0], 1
    for v in vals[1:]:
        if v == curr:
            count += 1
        else:
            runs.append((curr, count))
            curr, count = v, 1
    runs.append((curr, count))
    return runs


def send_decode(ctx, encryptor, encoder, rgb, out_path):
    """homo/client_decode.cpp:122-153: per colour channel the run-length pairs of the image, each as two ciphertexts
    (value, count), channel after channel -- the stream server.server_decode reads.  Returns (width, height, pairs[3]),
    the five integers the reference writes to keys/params.txt (:95-98,149)."""
    h, w, _ = rgb.shape
    flat = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    pairs = []
    first = _seed_start(encryptor)
    with open(out_path, "wb") as f:
        for ch in range(3):
            runs = run_length_pairs(flat[:, ch])
            pairs.append(len(runs))
            _encrypt_values(ctx, encryptor, encoder, [x for run in runs for x in run], f)
    _seed_finish(encryptor, first, out_path)
    return w, h, pairs


def receive_decode(ctx, decryptor, encoder, in_path, width, height, clamp=True, decoded=None):
    """homo/client_decode.cpp:157-214: the decoded image, uint8 [height, width, 3] (position-major, channels interleaved:
    the order homo/server_decode.cpp:139-143 saves)"""
    return receive_pixels(ctx, decryptor, encoder, in_path, width, height, clamp, decoded)


class BatchEncoder:
    """seal::PolyCRTBuilder: n integers modulo t in the slots of one plaintext (include/fhe_hip.h "batched plaintext slots": t prime,
    t = 1 mod 2n; two rows of n/2 slots, flat order row 0 then row 1).  encode() feeds DeviceEncryptor.encrypt_plains, decode() reads
    Decryptor.decrypt_batch; the transforms modulo t run on the host (fhe_batch_encode / fhe_batch_decode)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.slot_count = ctx.n
        probe = np.zeros(ctx.n, dtype=np.uint64)
        self._run("fhe_batch_encode", probe[None])                     # refuses a plain modulus without slots here, not at the first use

    def _run(self, name, rows):
        import ctypes as C
        from . import _lib
        src = np.ascontiguousarray(rows, dtype=np.uint64)
        if src.ndim != 2 or src.shape[1] != self.ctx.n:
            raise ValueError("%s: expected [count, n = %d] values, got %r" % (name, self.ctx.n, src.shape))
        out = np.zeros_like(src)
        _lib.call(name, self.ctx.n, self.ctx.t, src.ctypes.data_as(C.c_void_p), src.shape[0], out.ctypes.data_as(C.c_void_p))
        return out

    def encode_host(self, slots):
        """[count, n] (or [n]) slot values below t -> plaintext coefficients, numpy uint64 of the same shape"""
        a = np.asarray(slots)
        return self._run("fhe_batch_encode", a[None])[0] if a.ndim == 1 else self._run("fhe_batch_encode", a)

    def encode(self, slots):
        """[count, n] slot values -> [count, n] device tensor of plaintext coefficients (DeviceEncryptor.encrypt_plains takes it)"""
        import torch
        a = np.asarray(slots)
        plain = self._run("fhe_batch_encode", a[None] if a.ndim == 1 else a)
        return torch.from_numpy(plain.view(np.int64)).to(self.ctx.device)

    def decode(self, plains):
        """[count, n] (or [n]) plaintext coefficients (Decryptor.decrypt_batch's result, or a device tensor) -> slot values, numpy uint64"""
        if hasattr(plains, "detach"):
            plains = plains.detach().cpu().contiguous().numpy().view(np.uint64)
        a = np.asarray(plains)
        return self._run("fhe_batch_decode", a[None])[0] if a.ndim == 1 else self._run("fhe_batch_decode", a)


# ---- position-packed 8x8 blocks (include/fhe_hip.h "integer linear maps across slot-packed ciphertexts"; circuits.packed_dct_plan) ----
def pack_blocks(channel, width, height, n, t=None):
    """[groups][64][n] slot values: block b of `channel` (raster order, as blocks_of) goes to group b // n, slot b % n; position 8 r + c of
    the block names the ciphertext of the group; unused slots are 0.  int64, or uint64 reduced modulo t when t is given (what
    BatchEncoder.encode takes)."""
    blocks = blocks_of(np.asarray(channel).astype(np.int64), width, height)
    groups = max(1, (len(blocks) + n - 1) // n)
    out = np.zeros((groups, 64, n), dtype=np.int64)
    for b, blk in enumerate(blocks):
        out[b // n, :, b % n] = blk
    return out if t is None else (out % np.int64(t)).astype(np.uint64)


def unpack_blocks(slots, width, height):
    """the inverse of pack_blocks: [groups][64][n] values -> [height - height % 8][width - width % 8]"""
    a = np.asarray(slots)
    bw, bh = width // 8, height // 8
    n = a.shape[-1]
    out = np.zeros((bh * 8, bw * 8), dtype=a.dtype)
    for b in range(bw * bh):
        j, i = divmod(b, bw)
        out[8 * j:8 * j + 8, 8 * i:8 * i + 8] = a[b // n, :, b % n].reshape(8, 8)
    return out


# ---- position-packed frames and tiles (include/fhe_hip.h "sparse integer maps across position-packed ciphertexts"; circuits.packed_resize_plans)
def pack_frames(frames, n, t=None):
    """[groups][planes][n] slot values: frame b of `frames` ([count, ...]: every frame flattened row-major to `planes` pixels) goes to
    group b // n, slot b % n; pixel p of the frame names the ciphertext; unused slots are 0.  int64, or uint64 reduced modulo t."""
    a = np.asarray(frames).astype(np.int64)
    a = a.reshape(a.shape[0], -1)
    groups = max(1, (a.shape[0] + n - 1) // n)
    out = np.zeros((groups, a.shape[1], n), dtype=np.int64)
    for g in range(groups):
        part = a[g * n:(g + 1) * n]
        out[g, :, :part.shape[0]] = part.T
    return out if t is None else (out % np.int64(t)).astype(np.uint64)


def unpack_frames(slots, count, shape=None):
    """the inverse of pack_frames: [groups][planes][n] values -> [count, planes], or [count] + shape"""
    a = np.asarray(slots)
    frames = a.transpose(0, 2, 1).reshape(-1, a.shape[1])[:count]
    return frames if shape is None else frames.reshape((count,) + tuple(shape))


def _halo(halo):
    return (int(halo), int(halo)) if np.isscalar(halo) else (int(halo[0]), int(halo[1]))


def pack_tiles(channel, core_w, core_h, halo, n, t=None):
    """[groups][planes][n] slot values of one image cut into tiles: tile b (raster order over ceil(W / core_w) x ceil(H / core_h) cores)
    goes to group b // n, slot b % n, as a frame of (core_h + 2 halo_y) x (core_w + 2 halo_x) pixels, row-major: its core with `halo`
    (a number, or (halo_x, halo_y)) pixels on every side, clamp-to-edge at the image border."""
    a = np.asarray(channel).astype(np.int64)
    h, w = a.shape
    hx, hy = _halo(halo)
    tw, th = (w + core_w - 1) // core_w, (h + core_h - 1) // core_h
    frames = np.empty((tw * th, core_h + 2 * hy, core_w + 2 * hx), dtype=np.int64)
    for b in range(tw * th):
        j, i = divmod(b, tw)
        ys = np.clip(np.arange(j * core_h - hy, (j + 1) * core_h + hy), 0, h - 1)
        xs = np.clip(np.arange(i * core_w - hx, (i + 1) * core_w + hx), 0, w - 1)
        frames[b] = a[np.ix_(ys, xs)]
    return pack_frames(frames, n, t)


def unpack_tiles(slots, width, height, core_w, core_h):
    """stitches tiles of core_w x core_h pixels ([groups][core_h * core_w][n], tile b in group b // n, slot b % n, raster order) into
    [height][width]; what a partial tile holds beyond the image is dropped"""
    a = np.asarray(slots)
    tw, th = (width + core_w - 1) // core_w, (height + core_h - 1) // core_h
    tiles = unpack_frames(a, tw * th, (core_h, core_w))
    out = np.zeros((th * core_h, tw * core_w), dtype=a.dtype)
    for b in range(tw * th):
        j, i = divmod(b, tw)
        out[j * core_h:(j + 1) * core_h, i * core_w:(i + 1) * core_w] = tiles[b]
    return out[:height, :width]


def descale(values, scale_bits, t):
    """slot values modulo t -> integers: centred modulo t, divided by 2^scale_bits, rounded half away from zero (int64 for t < 2^63)"""
    v = np.asarray(values).astype(object) % int(t)
    v = np.where(v > (int(t) - 1) // 2, v - int(t), v)
    half = (1 << scale_bits) >> 1
    mag = (np.abs(v) + half) >> scale_bits if scale_bits else np.abs(v)
    return (np.where(v < 0, -mag, mag)).astype(np.int64)
