"""Reference of the baseline JPEG encoder (include/demonet_hip.h, dn_jpeg_encode and dn_jpeg_items_from_index) in numpy and plain
integers: the component planes of an item (through tests/compose_ref.py: a 1:1 item into an I420 BT.601 full-range surface), the edge rule, the
integer forward DCT, the quality-scaled Annex K quantisation, the Annex K Huffman tables, one restart interval per MCU row, the file around it, the
placement of the files in the arena and the device-built item table. Nothing here is fitted to device output; the tables are the ones ITU-T T.81
Annex K prints, and tests/test_jpeg.py holds them against the ones an independent encoder writes into its files. A minimal decoder for this subset
is at the end. The keyword `mistake` makes the classic wrong encoders (tests only):

    no_stuffing    no 0x00 behind a 0xFF data byte
    no_zrl         a zero run of 16 or more is not split: its low four bits go into the symbol
    rst_mod16      RSTm counted mod 16 instead of mod 8
    dc_keep        the DC predictors are not reset at a restart
    edge_zero      samples beyond a component plane are 0 instead of the plane's last column / row
    quant_trunc    the quantiser truncates toward zero
    swap_cbcr      Cb and Cr exchanged
    pad_zero       the last byte of an interval padded with 0-bits
"""
import numpy as np

import compose_ref as cr

MISTAKES = ("no_stuffing", "no_zrl", "rst_mod16", "dc_keep", "edge_zero", "quant_trunc", "swap_cbcr", "pad_zero")
YUV = ("nv12", "i420")
HEADER_BYTES = 613
MAX_ITEMS = 8192
OK, EMPTY, REFUSED, NO_SPACE = 0, 1, 2, 3

# ---------------------------------------------------------------------------------------------------------------- tables (T.81 Annex K)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
                   50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])       # natural index of zigzag position k
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFF = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)          # the order of the DHT segment; classes / ids (0, 0), (1, 0), (0, 1), (1, 1)


def huff_codes(table):
    """{symbol: (code, length)} of a (bits, values) table: T.81 Annex C"""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


CODES = [huff_codes(t) for t in HUFF]


def quant_tables(q):
    """(luma [64], chroma [64]) in natural order at quality q = 1 .. 100: the IJG rule in integers"""
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (Q_LUMA, Q_CHROMA))


# ---------------------------------------------------------------------------------------------------------------- the transform
CONST_BITS, PASS1_BITS, DCT_SCALE = 13, 2, 8


def _fix(c):
    return int(np.floor(c * (1 << CONST_BITS) + 0.5))


_C = [np.cos(k * np.pi / 16) for k in range(8)]
_R2 = np.sqrt(2.0)
F_0_298 = _fix(_R2 * (-_C[1] + _C[3] + _C[5] - _C[7]))
F_0_390 = _fix(_R2 * (_C[3] - _C[5]))
F_0_541 = _fix(_R2 * _C[6])
F_0_765 = _fix(_R2 * (_C[2] - _C[6]))
F_0_899 = _fix(_R2 * (_C[3] - _C[7]))
F_1_175 = _fix(_R2 * _C[3])
F_1_501 = _fix(_R2 * (_C[1] + _C[3] - _C[5] - _C[7]))
F_1_847 = _fix(_R2 * (_C[2] + _C[6]))
F_1_961 = _fix(_R2 * (_C[3] + _C[5]))
F_2_053 = _fix(_R2 * (_C[1] + _C[3] - _C[5] + _C[7]))
F_2_562 = _fix(_R2 * (_C[1] + _C[3]))
F_3_072 = _fix(_R2 * (_C[1] + _C[3] + _C[5] - _C[7]))
DCT_CONSTANTS = (F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175, F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n            # >> of a signed value: arithmetic (floor)


def _pass(d, first):
    """one 1-D pass of the Loeffler-Ligtenberg-Moschytz transform over the LAST axis of an int64 array [..., 8]"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
        n = CONST_BITS - PASS1_BITS
    else:
        out[0], out[4] = _descale(t10 + t11, PASS1_BITS), _descale(t10 - t11, PASS1_BITS)
        n = CONST_BITS + PASS1_BITS
    z1 = (t12 + t13) * F_0_541
    out[2], out[6] = _descale(z1 + t13 * F_0_765, n), _descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, -1)


def fdct(blocks):
    """[..., 8, 8] level-shifted samples (int) -> [..., 8, 8] int64 coefficients, DCT_SCALE = 8 times the orthonormal 2-D DCT: rows first (scaled up by
    2^PASS1_BITS), then columns. 13-bit constants round(c 2^13) of the closed-form cosines above; every intermediate fits 32 bits."""
    rows = _pass(np.asarray(blocks, np.int64), True)
    return np.swapaxes(_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantise(coef, table, mistake=None):
    """sign(c) ((|c| + d / 2) / d) with d = Q * DCT_SCALE; coef [..., 8, 8], table [64] natural order"""
    d = (table * DCT_SCALE).reshape(8, 8)
    a = np.abs(coef)
    return np.sign(coef) * ((a if mistake == "quant_trunc" else a + d // 2) // d)


# ---------------------------------------------------------------------------------------------------------------- planes of an item
def planewise(fmt, matrix, full):
    return fmt in YUV and matrix == "bt601" and bool(full)


def item_planes(fmt, matrix, full, planes, rect):
    """(Y [h, w], Cb [ceil(h/2), ceil(w/2)], Cr) uint8 of the rectangle (x0, y0, w, h) of one frame given as its payload planes: what a 1:1
    Compositor item into an I420 BT.601 full-range surface of w x h holds"""
    x0, y0, w, h = rect
    ch, cw = (h + 1) // 2, (w + 1) // 2
    dst = [[np.zeros((h, w), np.uint8), np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8)]]
    out = cr.compose([planes], dst, [(0, (x0, y0, w, h), 0, (0, 0, w, h))], (fmt, matrix, bool(full)), ("i420", "bt601", True))
    return out[0]


def mcu_blocks(plane, bw, bh, mistake=None):
    """[bh, bw, 8, 8] int64 level-shifted blocks of a component plane padded to bh x bw blocks: the last column and row replicated"""
    h, w = plane.shape
    if mistake == "edge_zero":
        p = np.zeros((bh * 8, bw * 8), np.int64)
        p[:h, :w] = plane
    else:
        p = np.asarray(plane, np.int64)[np.minimum(np.arange(bh * 8), h - 1)][:, np.minimum(np.arange(bw * 8), w - 1)]
    return (p - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)


def coefficients(Y, Cb, Cr, q, mistake=None):
    """the quantised coefficients ([2 my, 2 mx, 8, 8], [my, mx, 8, 8], [my, mx, 8, 8]) in natural order"""
    h, w = Y.shape
    mx, my = (w + 15) // 16, (h + 15) // 16
    ql, qc = quant_tables(q)
    return (quantise(fdct(mcu_blocks(Y, 2 * mx, 2 * my, mistake)), ql, mistake), quantise(fdct(mcu_blocks(Cb, mx, my, mistake)), qc, mistake),
            quantise(fdct(mcu_blocks(Cr, mx, my, mistake)), qc, mistake))


# ---------------------------------------------------------------------------------------------------------------- entropy coding
def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, cat):
    return v if v >= 0 else v + (1 << cat) - 1


def code_block(zz, pred, dc, ac, syms, stats, mistake=None):
    """append the (bits, length) pairs of one block (zz: 64 quantised values in zigzag order) to syms"""
    diff = int(zz[0]) - pred
    cat = _category(diff)
    stats["dc_cat"] = max(stats["dc_cat"], cat)
    c, n = dc[cat]
    syms.append(((c << cat) | _value_bits(diff, cat), n + cat))
    nz = np.nonzero(zz[1:])[0] + 1
    last = 0
    for k in nz:
        k = int(k)
        run = k - last - 1
        last = k
        v = int(zz[k])
        cat = _category(v)
        stats["ac_cat"] = max(stats["ac_cat"], cat)
        if mistake == "no_zrl":
            run &= 15
        while run >= 16:
            syms.append(ac[0xF0])
            stats["zrl"] += 1
            run -= 16
        c, n = ac[(run << 4) | cat]
        syms.append(((c << cat) | _value_bits(v, cat), n + cat))
    if last < 63:
        syms.append(ac[0x00])
    if len(nz) == 0:
        stats["eob_only"] += 1


def pack(syms, mistake=None):
    """the (bits, length) pairs MSB first, the last byte padded with 1-bits, a 0x00 behind every 0xFF; returns (bytes, stuffed count)"""
    if not syms:
        return b"", 0
    a = np.array(syms, np.int64)
    codes, lens = a[:, 0], a[:, 1]
    total = int(lens.sum())
    starts = np.cumsum(lens) - lens
    idx = np.repeat(np.arange(len(lens)), lens)
    off = np.arange(total) - starts[idx]
    bits = ((codes[idx] >> (lens[idx] - 1 - off)) & 1).astype(np.uint8)
    pad = (-total) % 8
    bits = np.concatenate([bits, np.full(pad, 0 if mistake == "pad_zero" else 1, np.uint8)])
    raw = np.packbits(bits)
    ff = raw == 0xFF
    if mistake == "no_stuffing" or not ff.any():
        return raw.tobytes(), int(ff.sum())
    out = np.zeros(len(raw) + int(ff.sum()), np.uint8)
    out[np.arange(len(raw)) + np.cumsum(ff) - ff] = raw
    return out.tobytes(), int(ff.sum())


def header(w, h, q):
    """SOI, APP0, DQT, SOF0, DHT, DRI, SOS: HEADER_BYTES bytes"""
    ql, qc = quant_tables(q)
    be = lambda v: bytes([v >> 8, v & 255])      # noqa: E731
    out = b"\xff\xd8" + b"\xff\xe0" + be(16) + b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    out += b"\xff\xdb" + be(2 + 65 * 2) + b"\x00" + bytes(int(v) for v in ql[ZIGZAG]) + b"\x01" + bytes(int(v) for v in qc[ZIGZAG])
    out += b"\xff\xc0" + be(17) + b"\x08" + be(h) + be(w) + b"\x03" + b"\x01\x22\x00" + b"\x02\x11\x01" + b"\x03\x11\x01"
    dht = b""
    for (bits, vals), tc_th in zip(HUFF, (0x00, 0x10, 0x01, 0x11)):
        dht += bytes([tc_th]) + bytes(bits) + bytes(vals)
    out += b"\xff\xc4" + be(2 + len(dht)) + dht
    out += b"\xff\xdd" + be(4) + be((w + 15) // 16)
    out += b"\xff\xda" + be(12) + b"\x03" + b"\x01\x00" + b"\x02\x11" + b"\x03\x11" + b"\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return out


def encode_planes(Y, Cb, Cr, q, mistake=None):
    """(the file, the counters) of one item given as its component planes"""
    h, w = Y.shape
    if mistake == "swap_cbcr":
        Cb, Cr = Cr, Cb
    cy, cb, cr_ = coefficients(Y, Cb, Cr, q, mistake)
    mx, my = (w + 15) // 16, (h + 15) // 16
    zy = cy.reshape(2 * my, 2 * mx, 64)[..., ZIGZAG]
    zb, zr = cb.reshape(my, mx, 64)[..., ZIGZAG], cr_.reshape(my, mx, 64)[..., ZIGZAG]
    stats = dict(stuffed=0, zrl=0, eob_only=0, dc_cat=0, ac_cat=0, mcu_rows=my, mcus_per_row=mx)
    out = [header(w, h, q)]
    pred = [0, 0, 0]
    for r in range(my):
        if mistake != "dc_keep":
            pred = [0, 0, 0]
        syms = []
        for m in range(mx):
            for by, bx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                z = zy[2 * r + by, 2 * m + bx]
                code_block(z, pred[0], CODES[0], CODES[1], syms, stats, mistake)
                pred[0] = int(z[0])
            for c, z in ((1, zb[r, m]), (2, zr[r, m])):
                code_block(z, pred[c], CODES[2], CODES[3], syms, stats, mistake)
                pred[c] = int(z[0])
        data, stuffed = pack(syms, mistake)
        stats["stuffed"] += stuffed
        out.append(data)
        if r < my - 1:
            out.append(bytes([0xFF, 0xD0 + r % (16 if mistake == "rst_mod16" else 8)]))
    out.append(b"\xff\xd9")
    stats["coefficients"] = (cy, cb, cr_)
    return b"".join(out), stats


def encode_item(fmt, matrix, full, planes, rect, q, mistake=None):
    """(the file, the counters) of the rectangle (x0, y0, w, h) of a frame given as its payload planes"""
    Y, Cb, Cr = item_planes(fmt, matrix, full, planes, rect)
    return encode_planes(Y, Cb, Cr, q, mistake)


# ---------------------------------------------------------------------------------------------------------------- the arena
def align16(v):
    return (v + 15) & ~15


def place(lengths, arena_bytes):
    """lengths: per slot the file length, or EMPTY / REFUSED / NO_SPACE as a negative status -1 / -2 / -3 for a slot without a file. Returns (results
    [n][4] (offset, length, status, 0), totals (written, refused, bytes_used, 0)): offset_i is the sum of align16(length_j) over every encodable
    j < i whether or not j fitted; i is written iff offset_i + length_i <= arena_bytes."""
    res = np.zeros((len(lengths), 4), np.int64)
    off = written = refused = used = 0
    for i, n in enumerate(lengths):
        if n < 0:
            res[i] = (0, 0, -n, 0)
            refused += -n != EMPTY
            continue
        if off + n <= arena_bytes:
            res[i] = (off, n, OK, 0)
            written += 1
            used = off + n
        else:
            res[i] = (off, 0, NO_SPACE, 0)
            refused += 1
        off += align16(n)
    return res.astype(np.int32), np.array([written, refused, used, 0], np.int32)


def arena_after(before, files, results):
    """the arena's bytes after a call: `before` with every written file at its offset"""
    out = np.array(before, np.uint8)
    for f, (off, n, status, _) in zip(files, results):
        if status == OK:
            assert len(f) == n
            out[off:off + n] = np.frombuffer(f, np.uint8)
    return out


def items_from_index(index, sizes, yuv, select, max_segments):
    """dn_jpeg_items_from_index: per index row (stream, row, x0, y0, width, height, 0, 0) the pair (status, (frame, x0, y0, w, h) or None).
    sizes[frame] = (height, width); select: None or one flag per row."""
    out, seg = [], 0
    for s, row in enumerate(np.asarray(index).tolist()):
        f, _, x0, y0, w, h = row[:6]
        if f == -1 or (select is not None and not select[s]):
            out.append((EMPTY, None))
            continue
        if f < 0 or f >= len(sizes) or w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > sizes[f][1] or y0 + h > sizes[f][0]:
            out.append((REFUSED, None))
            continue
        if yuv:
            w, h, x0, y0 = w + (x0 & 1), h + (y0 & 1), x0 & ~1, y0 & ~1
        rows = (h + 15) // 16
        if seg + rows > max_segments:
            out.append((NO_SPACE, None))
        else:
            out.append((OK, (f, x0, y0, w, h)))
        seg += rows
    return out


# ---------------------------------------------------------------------------------------------------------------- a decoder for this subset
def _idct_basis():
    k, x = np.arange(8)[:, None], np.arange(8)[None, :]
    m = np.cos((2 * x + 1) * k * np.pi / 16) * 0.5
    m[0] /= np.sqrt(2.0)
    return m            # [k][x]: orthonormal


_BASIS = _idct_basis()


def dct_float(blocks):
    """the orthonormal 2-D DCT in float64 (what fdct approximates, times DCT_SCALE)"""
    return _BASIS @ np.asarray(blocks, np.float64) @ _BASIS.T


def idct_float(coef):
    return _BASIS.T @ np.asarray(coef, np.float64) @ _BASIS


class _Bits:
    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(data, np.uint8)).tolist()
        self.at = 0

    def take(self, n):
        v = 0
        for b in self.bits[self.at:self.at + n]:
            v = (v << 1) | b
        assert self.at + n <= len(self.bits), "the interval ran out of bits"
        self.at += n
        return v

    def symbol(self, lookup):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (code, length) in lookup:
                return lookup[(code, length)]
        raise AssertionError("no such code")


def _extend(v, cat):
    return v if cat == 0 or v >= (1 << (cat - 1)) else v - (1 << cat) + 1


def decode(data):
    """A baseline 4:2:0 JFIF file of this encoder's shape -> dict(width, height, q=(luma [64], chroma [64]) natural order, coefficients=(Y [2my, 2mx,
    8, 8], Cb, Cr) quantised, planes=(Y, Cb, Cr) float64 pixel planes of the padded size, restart markers seen). AssertionError for anything else."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    at, q, huff, dri, w, h = 2, {}, {}, 0, 0, 0
    while True:
        assert data[at] == 0xFF
        marker, n = data[at + 1], (data[at + 2] << 8) | data[at + 3]
        seg = data[at + 4:at + 2 + n]
        at += 2 + n
        if marker == 0xDB:
            while seg:
                assert seg[0] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(seg[1:65])
                q[seg[0] & 15] = t
                seg = seg[65:]
        elif marker == 0xC0:
            assert seg[0] == 8 and seg[5] == 3 and bytes(seg[6:15]) == b"\x01\x22\x00\x02\x11\x01\x03\x11\x01"
            h, w = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
        elif marker == 0xC4:
            while seg:
                bits = list(seg[1:17])
                cnt = sum(bits)
                huff[seg[0]] = {v: k for k, v in huff_codes((bits, list(seg[17:17 + cnt]))).items()}
                seg = seg[17 + cnt:]
        elif marker == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif marker == 0xDA:
            assert bytes(seg) == b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
            break
        else:
            assert marker == 0xE0
    mx, my = (w + 15) // 16, (h + 15) // 16
    assert dri == mx
    body = data[at:-2]
    intervals, markers, start, i = [], [], 0, 0
    while i < len(body):
        if body[i] == 0xFF:
            assert i + 1 < len(body)
            if body[i + 1] == 0:
                i += 2
                continue
            assert 0xD0 <= body[i + 1] <= 0xD7, "marker {:02x} inside the scan".format(body[i + 1])
            intervals.append(body[start:i])
            markers.append(body[i + 1] - 0xD0)
            i += 2
            start = i
        else:
            i += 1
    intervals.append(body[start:])
    assert len(intervals) == my and markers == [r % 8 for r in range(my - 1)]
    cy, cb, cr_ = np.zeros((2 * my, 2 * mx, 64), np.int64), np.zeros((my, mx, 64), np.int64), np.zeros((my, mx, 64), np.int64)
    for r, iv in enumerate(intervals):
        rd = _Bits(iv.replace(b"\xff\x00", b"\xff"))
        pred = [0, 0, 0]
        for m in range(mx):
            for c, (dst, dc, ac) in enumerate(((None, 0x00, 0x10), (cb[r, m], 0x01, 0x11), (cr_[r, m], 0x01, 0x11))):
                for blk in (range(4) if c == 0 else range(1)):
                    z = cy[2 * r + (blk >> 1), 2 * m + (blk & 1)] if c == 0 else dst
                    cat = rd.symbol(huff[dc])
                    pred[c] += _extend(rd.take(cat), cat)
                    z[0] = pred[c]
                    k = 1
                    while k < 64:
                        s = rd.symbol(huff[ac])
                        run, cat = s >> 4, s & 15
                        if cat == 0:
                            if run != 15:
                                assert run == 0
                                break
                            k += 16
                            continue
                        k += run
                        assert k < 64
                        z[k] = _extend(rd.take(cat), cat)
                        k += 1
        left = rd.bits[rd.at:]
        assert len(left) < 8 and all(left), "an interval ends with at most seven 1-bits"
    unz = np.argsort(ZIGZAG)
    coef = tuple(c[..., unz].reshape(c.shape[0], c.shape[1], 8, 8) for c in (cy, cb, cr_))
    planes = []
    for c, t in zip(coef, (q[0], q[1], q[1])):
        px = idct_float(c * t.reshape(8, 8)) + 128.0
        planes.append(px.transpose(0, 2, 1, 3).reshape(c.shape[0] * 8, c.shape[1] * 8))
    return dict(width=w, height=h, q=(q[0], q[1]), coefficients=coef, planes=tuple(planes), markers=markers)


# ---------------------------------------------------------------------------------------------------------------- scenes
QUALITIES = (5, 50, 85, 100)
RECTS = [(0, 0, 1, 1), (4, 2, 16, 16), (20, 30, 17, 15), (64, 48, 33, 47)]          # even origins, inside the smaller noise surface


def checkerboard_planes():
    """payload planes (NV12) of the 32 x 32 0/255 checkerboard: squares of 8 in the upper half (neighbouring blocks differ by the whole DC range),
    the same squares moved by (4, 4) in the lower half (every block holds four quadrants: the largest AC values)"""
    yy, xx = np.mgrid[0:32, 0:32]
    upper = ((yy >> 3) + (xx >> 3)) & 1
    lower = (((yy + 4) >> 3) + ((xx + 4) >> 3)) & 1
    Y = (np.where(yy < 16, upper, lower) * 255).astype(np.uint8)
    cy, cx = np.mgrid[0:16, 0:16]
    U = ((((cy >> 3) + (cx >> 3)) & 1) * 255).astype(np.uint8)
    return [Y, cr.fr.interleave(U, 255 - U)]


def gradient_planes():
    """payload planes (NV12) of the 20 x 1048 gradient surface: 66 MCUs per row, 2 rows"""
    yy, xx = np.mgrid[0:20, 0:1048]
    Y = ((xx * 3 + yy * 5) & 255).astype(np.uint8)
    cy, cx = np.mgrid[0:10, 0:524]
    return [Y, cr.fr.interleave(((cx + 2 * cy) & 255).astype(np.uint8), ((3 * cx + cy + 90) & 255).astype(np.uint8))]


def flat_planes():
    return [np.full((48, 40), 131, np.uint8), np.full((24, 40), 77, np.uint8)]


def plane_scenes():
    """name -> (format, payload planes, rectangle) of the scenes every BT.601 full-range (plane-wise) check runs on"""
    import regions_ref as rr
    out = {}
    for i, (h, w) in enumerate(rr.SIZES):
        out["noise{}".format(i)] = ("nv12", cr.noise_planes("nv12", 940 + i, h, w), (0, 0, w, h))
    for r in RECTS:
        out["rect{}x{}".format(r[2], r[3])] = ("nv12", cr.noise_planes("nv12", 941, *rr.SIZES[1]), r)
    out["gradient"] = ("nv12", gradient_planes(), (0, 0, 1048, 20))
    out["flat"] = ("nv12", flat_planes(), (0, 0, 40, 48))
    out["checkerboard"] = ("nv12", checkerboard_planes(), (0, 0, 32, 32))
    return out
