"""Baseline (SOF0) JPEG streams written from quantised coefficient blocks the caller supplies -- the streams Pillow's encoder
cannot write: any component ids and SOS selector order, per-component DC / AC table choice, arbitrary Huffman tables
(16-bit codes, single-symbol tables), DQT with Pq 0 or 1, JFIF / Adobe markers present or not, any restart interval and
0xFF fill bytes in front of markers.  Test helper (imported by the JPEG tests), not part of the product.

Coefficients: ``coefs[c]`` is an int array [rows][cols][64] (natural order, quantised) of component c's blocks, rows =
MCU rows x v, cols = MCU columns x h.  ``mcu_blocks(coefs, comps)`` lists them the way the decoders return them
(MCUs in raster order, inside an MCU the components in SOF order, a component's blocks row by row)."""
import itertools

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K.3 tables (bits[1..16], values)
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

ALL_AC = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]      # every baseline AC symbol (162)
ALL_DC = list(range(12))


def table_from_lengths(lengths):
    """{symbol: code length} -> (bits, values) of a canonical table.  Kraft sum must stay < 1 (no all-ones code)."""
    assert sum(2.0 ** -l for l in lengths.values()) < 1.0 and all(1 <= l <= 16 for l in lengths.values())
    bits = [0] * 16
    for l in lengths.values():
        bits[l - 1] += 1
    vals = [s for s, _ in sorted(lengths.items(), key=lambda kv: (kv[1], kv[0]))]
    return bits, vals


def long_code_table(symbols, long_symbols, long_len=16):
    """A table in which `long_symbols` get codes of `long_len` bits (beyond any look-ahead) and the other `symbols` short
    ones: the short codes fill a complete-minus-margin prefix tree, the long ones hang off its last free branch."""
    short = [s for s in symbols if s not in long_symbols]
    n = len(short)
    ls = max(1, int(np.ceil(np.log2(n + 1))) + 1)             # enough room for n codes plus a free branch
    lengths = {s: ls for s in short}
    lengths.update({s: long_len for s in long_symbols})
    return table_from_lengths(lengths)


def _codes(table):
    bits, vals = table
    code, k, out = 0, 0, {}
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def _category(v):
    return 0 if v == 0 else int(abs(int(v))).bit_length()


def _magnitude(v, s):
    return v if v >= 0 else v + (1 << s) - 1


class _BitWriter(object):
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, length):
        assert 0 <= value < (1 << length) or length == 0
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):                                   # pad with 1-bits to the byte boundary (T.81 F.1.2.3)
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)


class Comp(object):
    def __init__(self, cid, h=1, v=1, tq=0, td=0, ta=0):
        self.id, self.h, self.v, self.tq, self.td, self.ta = cid, h, v, tq, td, ta


def geometry(width, height, comps):
    hmax, vmax = max(c.h for c in comps), max(c.v for c in comps)
    if len(comps) == 1:
        hmax = vmax = 1
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    return hmax, vmax, mcux, mcuy


def block_shapes(width, height, comps):
    """[rows, cols] of blocks of each component (whole MCUs)."""
    _, _, mcux, mcuy = geometry(width, height, comps)
    if len(comps) == 1:
        return [(mcuy, mcux)]
    return [(mcuy * c.v, mcux * c.h) for c in comps]


def mcu_blocks(coefs, comps, width, height):
    """The blocks in the order the decoders return them: [blocks][64] int16."""
    _, _, mcux, mcuy = geometry(width, height, comps)
    hv = [(1, 1)] if len(comps) == 1 else [(c.h, c.v) for c in comps]
    out = []
    for my in range(mcuy):
        for mx in range(mcux):
            for c, (h, v) in enumerate(hv):
                for by in range(v):
                    for bx in range(h):
                        out.append(coefs[c][my * v + by, mx * h + bx])
    return np.array(out, np.int16)


def forge(width, height, comps, coefs, qtables, dc_tables, ac_tables, scan_order=None, jfif=True, adobe=None, restart=0,
          fill=0, pq=None, sof=0xC0, extra_head=b''):
    """-> bytes of one baseline JPEG.

    comps: list of Comp in SOF order (id, sampling, tq, and the td / ta the SOS gives it).  coefs: per component
    [rows][cols][64] natural order.  qtables: {id: 64 values, natural order}; dc_tables / ac_tables: {id: (bits, values)}.
    scan_order: SOS component order as indices into comps (default: SOF order).  adobe: None or the APP14 transform
    byte.  restart: DRI interval in MCUs (0 = none).  fill: 0xFF fill bytes written in front of every RSTn and the EOI.
    pq: {id: 0 / 1} precision per quantisation table (default 0)."""
    n = len(comps)
    scan_order = list(range(n)) if scan_order is None else list(scan_order)
    hmax, vmax, mcux, mcuy = geometry(width, height, comps)
    out = bytearray(b'\xff\xd8')
    if jfif:
        out += _seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    if adobe is not None:
        out += _seg(0xEE, b'Adobe' + bytes([0, 100, 0, 0, 0, 0, adobe]))
    out += extra_head
    for tid, q in sorted(qtables.items()):
        p = (pq or {}).get(tid, 0)
        zz = [int(q[ZIGZAG[k]]) for k in range(64)]
        body = bytes([(p << 4) | tid]) + (b''.join(v.to_bytes(2, 'big') for v in zz) if p else bytes(zz))
        out += _seg(0xDB, body)
    out += _seg(sof, bytes([8]) + height.to_bytes(2, 'big') + width.to_bytes(2, 'big') + bytes([n]) +
                b''.join(bytes([c.id, (c.h << 4) | c.v, c.tq]) for c in comps))
    for tc, tabs in ((0, dc_tables), (1, ac_tables)):
        for tid, (bits, vals) in sorted(tabs.items()):
            out += _seg(0xC4, bytes([(tc << 4) | tid]) + bytes(bits) + bytes(vals))
    if restart:
        out += _seg(0xDD, restart.to_bytes(2, 'big'))
    out += _seg(0xDA, bytes([n]) + b''.join(bytes([comps[i].id, (comps[i].td << 4) | comps[i].ta]) for i in scan_order) +
                bytes([0, 63, 0]))
    dcc = {t: _codes(tab) for t, tab in dc_tables.items()}
    acc = {t: _codes(tab) for t, tab in ac_tables.items()}
    hv = [(1, 1)] if n == 1 else [(c.h, c.v) for c in comps]
    w = _BitWriter()
    pred = [0] * n
    rst = 0
    for m in range(mcux * mcuy):
        if restart and m and m % restart == 0:
            w.flush()
            out += w.out
            w.out = bytearray()
            out += b'\xff' * fill + bytes([0xFF, 0xD0 + (rst & 7)])
            rst += 1
            pred = [0] * n
        my, mx = divmod(m, mcux)
        for c in scan_order:
            h, v = hv[c]
            dct, act = dcc[comps[c].td], acc[comps[c].ta]
            for by in range(v):
                for bx in range(h):
                    blk = np.asarray(coefs[c][my * v + by, mx * h + bx]).astype(np.int64)
                    zz = blk[ZIGZAG]
                    diff = int(zz[0]) - pred[c]
                    pred[c] = int(zz[0])
                    s = _category(diff)
                    code, l = dct[s]
                    w.put(code, l)
                    if s:
                        w.put(_magnitude(diff, s), s)
                    run = 0
                    last = max([k for k in range(1, 64) if zz[k]] or [0])
                    for k in range(1, last + 1):
                        if zz[k] == 0:
                            run += 1
                            continue
                        while run > 15:
                            code, l = act[0xF0]
                            w.put(code, l)
                            run -= 16
                        s = _category(zz[k])
                        assert 1 <= s <= 10, 'AC coefficient %d out of the baseline range' % zz[k]
                        code, l = act[(run << 4) | s]
                        w.put(code, l)
                        w.put(_magnitude(int(zz[k]), s), s)
                        run = 0
                    if last < 63:
                        code, l = act[0x00]
                        w.put(code, l)
    w.flush()
    out += w.out
    out += b'\xff' * fill + b'\xff\xd9'
    return bytes(out)


def std_tables(ncomp):
    """Annex K tables: DC / AC 0 (luma) and 1 (chroma)."""
    if ncomp == 1:
        return {0: STD_DC_LUMA}, {0: STD_AC_LUMA}
    return {0: STD_DC_LUMA, 1: STD_DC_CHROMA}, {0: STD_AC_LUMA, 1: STD_AC_CHROMA}


def random_coefs(rng, width, height, comps, amp=40, density=0.25, dc_amp=60):
    """Coefficient planes of plausible size: DC values drifting around zero, sparse AC values decaying with frequency."""
    out = []
    freq = (np.arange(64) // 8) + (np.arange(64) % 8)
    for rows, cols in block_shapes(width, height, comps):
        a = np.zeros((rows, cols, 64), np.int64)
        a[..., 0] = rng.integers(-dc_amp, dc_amp + 1, (rows, cols))
        scale = np.maximum(1, amp / (1 + freq))
        ac = np.rint(rng.normal(0, 1, (rows, cols, 64)) * scale).astype(np.int64)
        mask = rng.random((rows, cols, 64)) < density
        a[..., 1:] = (ac * mask)[..., 1:]
        a[..., 1:] = np.clip(a[..., 1:], -1023, 1023)
        out.append(a)
    return out


# ---- stream families shared by the CPU and GPU JPEG tests --------------------------------------------------------------
LAYOUTS = {'grey': [(1, 1)], '444': [(1, 1)] * 3, '422': [(2, 1), (1, 1), (1, 1)], '420': [(2, 2), (1, 1), (1, 1)]}


def comps_for(layout, ids=(1, 2, 3), swap=False):
    hv = LAYOUTS[layout]
    t = [1, 0, 0] if swap else [0, 1, 1]
    return [Comp(ids[c], h, v, tq=min(c, 1), td=t[c], ta=t[c]) for c, (h, v) in enumerate(hv)]


def std_q(ncomp, v0=3, v1=5):
    q = {0: np.full(64, v0)}
    if ncomp == 3:
        q[1] = np.full(64, v1)
    return q


def restart_streams(seed=0):
    """restart intervals that end on a long symbol (a 16-bit AC code + 10 magnitude bits at k = 63), every scan alignment
    (COM segments of 0..3 bytes in front of the scan), intervals of 1..3 MCUs"""
    rng = np.random.default_rng(seed)
    comps = [Comp(1)]
    dc, _ = std_tables(1)
    ac = long_code_table(ALL_AC, [0xEA])                  # run 14 / size 10: the symbol that reaches k = 63
    out = []
    for ri in (1, 2, 3):
        for pad in range(4):
            for _ in range(3):
                w, h = 8 * int(rng.integers(3, 9)), 8 * int(rng.integers(1, 4))
                co = random_coefs(rng, w, h, comps, amp=20, density=0.2)
                co[0][..., 1:] *= (rng.random(co[0].shape[:2] + (1,)) < 0.5)
                for k in range(48, 63):
                    co[0][..., ZIGZAG[k]] = 0
                co[0][..., 63] = rng.choice([-1, 1], co[0].shape[:2]) * rng.integers(512, 1024, co[0].shape[:2])
                com = b'\xff\xfe' + (2 + pad).to_bytes(2, 'big') + b'x' * pad
                out.append(forge(w, h, comps, co, {0: np.full(64, 2)}, dc, {0: ac}, restart=ri, fill=int(rng.integers(0, 2)),
                                   extra_head=com))
    return out


def id_matrix():
    """{JFIF} x {Adobe none / 0 / 1} x {ids 1-2-3, 'R'-'G'-'B', other} x {scan in SOF order, permuted} x {td/ta swapped}:
    (stream, expected rgb flag by libjpeg's rule, permuted) -- 4:2:0 frames, DC / AC tables that differ per class"""
    rng = np.random.default_rng(41)
    dc, ac = std_tables(3)
    out = []
    for jfif, adobe, ids, perm, swap in itertools.product((True, False), (None, 0, 1), ((1, 2, 3), (82, 71, 66), (7, 40, 200)),
                                                         (False, True), (False, True)):
        comps = comps_for('420', ids, swap)
        w, h = 24, 16
        co = random_coefs(rng, w, h, comps)
        d = forge(w, h, comps, co, std_q(3), dc, ac, scan_order=[0, 2, 1] if perm else None, jfif=jfif, adobe=adobe)
        rgb = False if jfif else (adobe == 0 if adobe is not None else ids == (82, 71, 66))
        out.append((d, rgb, perm, (jfif, adobe, ids, perm, swap)))
    return out


def edge_streams():
    """Huffman and coefficient edges: DC categories 0..11 with predictors running across MCUs, ZRL runs, the last
    coefficient at k = 62 (EOB at 63) and at k = 63 (no EOB), 16-bit codes beyond both look-ahead widths, single-symbol
    tables"""
    rng = np.random.default_rng(42)
    out = []
    dc_long = long_code_table(ALL_DC, [10, 11])               # categories 10 / 11 get 16-bit DC codes (> GJ_DC_BITS)
    ac_long = long_code_table(ALL_AC, [0xF0, 0x00, 0x3A, 0xEA, 0x11])      # ZRL, EOB and others at 16 bits (> GJ_AC_BITS)
    for layout in ('grey', '444', '420'):
        comps = comps_for(layout)
        n = len(comps)
        w, h = 48, 32
        co = random_coefs(rng, w, h, comps)
        for c in range(n):                                         # DC differences of every category 0..11, both signs
            flat = co[c][..., 0].reshape(-1)
            acc = 0
            for i in range(flat.size):
                cat = i % 12
                diff = 0 if cat == 0 else int(rng.choice([-1, 1])) * int(rng.integers(1 << (cat - 1), 1 << cat))
                if abs(acc + diff) > 2047:
                    diff = -diff
                acc += diff
                flat[i] = acc
            co[c][..., 0] = flat.reshape(co[c].shape[:2])
            blocks = co[c].reshape(-1, 64)
            for i in range(blocks.shape[0]):
                kind = i % 5
                zz = np.zeros(64, np.int64)
                if kind == 0:                                      # ZRL runs: nonzero at zigzag 1, 18, 35, 52
                    zz[[1, 18, 35, 52]] = rng.integers(1, 400, 4)
                elif kind == 1:                                    # last coefficient at 62: EOB at k = 63
                    zz[[5, 62]] = (-3, 1023)
                elif kind == 2:                                    # last coefficient at 63: no EOB
                    zz[[2, 63]] = (7, -1023)
                elif kind == 3:                                    # 47 zeros then one at 63 (three ZRL + run 15)
                    zz[[15, 63]] = (1, -2)
                else:                                              # dense
                    zz[1:] = rng.integers(-3, 4, 63)
                zz[0] = blocks[i, 0]
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = zz
                blocks[i] = nat
        for dct, act in ((std_tables(n)[0], std_tables(n)[1]), ({0: dc_long, 1: dc_long}, {0: ac_long, 1: ac_long})):
            dct = {k: v for k, v in dct.items() if k < min(n, 2)}
            act = {k: v for k, v in act.items() if k < min(n, 2)}
            for rst in (0, 3):
                out.append(forge(w, h, comps, co, std_q(n, 1, 2), dct, act, restart=rst))
    # single-symbol tables: DC category 0 only (every DC 0); AC symbol 0x01 only (all 63 coefficients +-1, no EOB) /
    # EOB only (DC-only blocks)
    for layout in ('grey', '422'):
        comps = comps_for(layout)
        n = len(comps)
        for acsym in (0x01, 0x00):
            co = []
            for rows, cols in block_shapes(24, 16, comps):
                a = np.zeros((rows, cols, 64), np.int64)
                if acsym == 0x01:
                    a[..., 1:] = rng.choice([-1, 1], (rows, cols, 63))
                co.append(a)
            tab_dc, tab_ac = ([1] + [0] * 15, [0]), ([1] + [0] * 15, [acsym])
            out.append(forge(24, 16, comps, co, std_q(n, 9, 17), {0: tab_dc, 1: tab_dc} if n > 1 else {0: tab_dc},
                               {0: tab_ac, 1: tab_ac} if n > 1 else {0: tab_ac}))
    return out


def qrange_streams():
    """8-bit quantisers with coefficients past every 16-bit limit of libjpeg-turbo's SIMD IDCT: dequantised values that
    wrap in the 16-bit multiply, DC shortcuts whose << PASS1_BITS wraps (DC x q > 8191), pass-1 sums that saturate,
    dense +-1023 blocks under random tables, DC values ramped up to +-32767 -- and the boundary cases in a single
    coefficient of a 16 x 16 grey frame at q = 255 (DC 32 / 33, AC at natural index 1: 30 / 40 / 100)"""
    rng = np.random.default_rng(43)
    out = []
    g = comps_for('grey')
    dc, ac = std_tables(1)
    for idx, val in ((0, 32), (0, 33), (0, -33), (1, 30), (1, 40), (1, 100), (1, -100), (8, 40), (9, 100)):
        a = np.zeros((2, 2, 64), np.int64)
        a[0, 0, idx] = val
        out.append(forge(16, 16, g, [a], {0: np.full(64, 255)}, dc, ac))
    for layout in ('grey', '420'):
        comps = comps_for(layout)
        n = len(comps)
        dc, ac = std_tables(n)
        for kind in range(6):
            co = []
            for rows, cols in block_shapes(32, 16, comps):
                a = np.zeros((rows, cols, 64), np.int64)
                if kind == 0:                                        # +-510 everywhere: inside every limit
                    a[..., :] = rng.integers(-2, 3, (rows, cols, 64))
                elif kind == 1:                                      # DC only, x 255 up to +-33150: the shortcut wraps
                    a[..., 0] = rng.integers(-130, 131, (rows, cols))
                elif kind == 2:                                      # row 0 only, up to +-1023 x 255: 16-bit products wrap
                    a[..., :8] = rng.integers(-1023, 1024, (rows, cols, 8))
                elif kind == 3:                                      # dense, large: 16-bit sums wrap, pass 1 saturates
                    a[..., :] = rng.integers(-1023, 1024, (rows, cols, 64))
                elif kind == 4:                                      # sparse extremes
                    m = rng.random((rows, cols, 64)) < 0.08
                    a[..., :] = np.where(m, rng.choice([-1023, 1023], (rows, cols, 64)), 0)
                else:                                                # DC ramped towards the int16 edge (below)
                    a[..., 9] = rng.integers(-3, 4, (rows, cols))
                co.append(a)
            if kind == 5:                                            # +-2000 per block in decode order (DC category 11)
                for c, a in enumerate(co):
                    order = [(r, k) for r in range(a.shape[0]) for k in range(a.shape[1])]
                    if n == 3:
                        h, v = comps[c].h, comps[c].v
                        order.sort(key=lambda rk: ((rk[0] // v) * (a.shape[1] // h) + rk[1] // h, rk[0] % v, rk[1] % h))
                    sign = 1 if c % 2 == 0 else -1
                    for i, (r, k) in enumerate(order):
                        a[r, k, 0] = sign * min(32767, 2000 * i)
            q = {0: rng.integers(1, 256, 64), 1: np.full(64, 255)} if kind in (3, 5) else std_q(n, 255, 255)
            out.append(forge(32, 16, comps, co, q if n == 3 else {0: q[0]}, dc, ac))
    return out


def with_size(data, w, h):
    i = data.index(b'\xff\xc0')
    return data[:i + 5] + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + data[i + 9:]
