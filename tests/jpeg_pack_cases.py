"""Inputs of the entropy-coder tests (tests/test_jpeg_pack_host.py on the host writer, tests/test_gpu_jpeg_pack.py on the device
coder): a crafted set of avcer_jpeg_plan descriptors with hand-written coefficients -- the writers code what they are given, so the
coefficients need not come from an image -- and a set of small images.  No test in here."""
import io

import numpy as np

from avcer_amd import jpeg

# zigzag position -> natural (row-major) index of a coefficient (csrc/jpeg.h kNatural)
NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
           57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
R_NO_SPACE, R_RANGE, R_ENC_DESC = 12, 16, 19


def _zz(pairs):
    """One block from {zigzag position: value}."""
    b = np.zeros(64, dtype=np.int16)
    for k, v in pairs.items():
        b[NATURAL[k]] = v
    return b


def crafted(lib):
    """(names, coefficients int16 [blocks, 64], DESC records, the status avcer_jpeg_write_batch must give every file).  Every file
    is one to four MCUs but the all-zero 64 x 64 one; a few hundred blocks in all."""
    files = []  # (name, w, h, subsampling, blocks [n, 64] in STORAGE order, expected status)

    def add(name, w, h, sub, blocks, status=0):
        files.append((name, w, h, sub, np.asarray(blocks, dtype=np.int16).reshape(-1, 64), status))

    good = [_zz({0: 3 * c + 1, 1: -2, 5: 7}) for c in range(3)]
    # only the last coefficient: 62 zeros = three ZRL and a run of 14; no EOB
    add("last coefficient only", 8, 8, 0, [_zz({63: 5}), _zz({63: -1}), _zz({0: 9, 63: 1023})])
    # zero runs of exactly 15 (no ZRL) and exactly 16 (one ZRL, run 0), in luma and in chroma
    add("runs of 15 and 16", 16, 8, 0, [_zz({16: 2, 33: -3}), _zz({17: 1, 33: 1}), _zz({16: -1, 33: 4}), _zz({}), _zz({17: 9}), _zz({16: 9, 32: 1})])
    # the longest block there is: the scratch bound
    for sign in (1, -1):
        add(f"every AC {sign * 1023}", 8, 8, 0, [_zz({k: (sign * 1023 if k else 0) for k in range(64)})] * 3)
        add(f"every AC {sign * 1023} behind the largest DC difference", 16, 8, 0,
            [_zz({k: (sign * 1023 if k else (-1024 if b % 2 else 1023)) for k in range(64)}) for b in range(6)])
    # DC differences of +-2047 inside an MCU and across MCUs, 4:2:0, two MCUs: luma storage is 2 rows of 4, MCU m holds columns 2 m, 2 m + 1
    hi, lo = 1023, -1024
    luma = np.zeros((2, 4), dtype=np.int64)
    luma[0, 0], luma[0, 1], luma[1, 0], luma[1, 1] = hi, lo, hi, hi      # 1023, -2047, +2047, 0
    luma[0, 2], luma[0, 3], luma[1, 2], luma[1, 3] = lo, hi, lo, lo      # -2047 across the MCUs, +2047, -2047, 0
    add("DC differences of 2047", 32, 16, 2, [_zz({0: v}) for v in luma.reshape(-1)] + [_zz({0: hi}), _zz({0: lo}), _zz({0: lo}), _zz({0: hi})])
    # eight different luma DCs: the order of prediction inside an MCU is not the order of storage
    add("4:2:0 prediction order", 32, 16, 2, [_zz({0: v}) for v in (10, -20, 300, -4, 77, -500, 6, 1)] + [_zz({0: c}) for c in (5, -5, 9, -9)])
    add("4:2:2 prediction order", 32, 8, 1, [_zz({0: v, 2: 1}) for v in (100, -3, 50, 8)] + [_zz({0: c}) for c in (5, -5, 9, -9)])
    # 96 blocks of 6 and 4 bits: many blocks per output byte, a 64-byte scan
    add("all zero 64 x 64", 64, 64, 2, np.zeros((96, 64)))
    # scans of 16, 17, ... 23 bits and 14, 22: every residue mod 8 (a luma DC of category k costs 2, 4, 5, 6, 7, 8, 10 bits)
    for k, cb in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (5, 1), (6, 0), (6, 1)):
        add(f"luma DC category {k}, Cb {cb}", 8, 8, 0, [_zz({0: (1 << k) >> 1}), _zz({0: cb}), _zz({})])
    # coefficients without a code, each between two good files
    add("good 0", 8, 8, 0, good)
    add("an AC of 1024", 8, 8, 0, [good[0], _zz({0: 1, 40: 1024}), good[2]], R_RANGE)
    add("good 1", 8, 8, 0, good)
    add("a DC difference of 2048", 16, 8, 0, [_zz({0: 1024}), _zz({0: -1024})] + good[:1] * 4, R_RANGE)
    add("good 2", 8, 8, 0, good)
    add("bw[0] off by one", 16, 16, 2, [good[0]] * 6, R_ENC_DESC)
    add("good 3", 17, 9, 1, [_zz({0: b, b + 1: b - 3}) for b in range(16)])

    desc = np.zeros(len(files), dtype=jpeg.DESC)
    at = 0
    for i, (name, w, h, sub, blocks, status) in enumerate(files):
        d, need = jpeg.plan(lib, [(w, h)], 95, sub)
        assert need == len(blocks), name
        desc[i] = d[0]
        desc[i]["coef_block"] = at
        at += need
        if name.startswith("bw[0]"):
            desc[i]["bw"][0] += 1
    coeffs = np.concatenate([f[4] for f in files])
    return [f[0] for f in files], coeffs, desc, np.array([f[5] for f in files], dtype=np.int32)


def subset(coeffs, desc, order):
    """The files `order` of a set as a set of their own: (coefficients, DESC records), blocks packed in that order."""
    d = desc[list(order)].copy()
    parts, at = [], 0
    for k, i in enumerate(order):
        a, n = int(desc[i]["coef_block"]), int(desc[i]["n_blocks"])
        parts.append(coeffs[a:a + n])
        d[k]["coef_block"] = at
        at += n
    return np.concatenate(parts), d


def _smooth(h, w, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([np.sin(xx / (5.0 + c + seed)) * 70 + np.cos(yy / (7.0 - c)) * 50 + 128 for c in range(3)], axis=2)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


SIZES = ((1, 1), (8, 8), (17, 13), (33, 16), (40, 40))  # (w, h)


def image_groups():
    """{(quality, subsampling): [rgb u8 [h, w, 3], ...]}: noise and a smooth gradient at every size of SIZES, for subsampling 0 / 1 / 2
    and quality 1 / 95 / 100 -- ten unequal images a group.  The group (95, 0) also holds the 8 x 8 noise of default_rng(8), whose
    file ends FF 00 FF D9, and (100, 0) the 40 x 40 noise of default_rng(0), which carries 37 stuffed bytes."""
    out = {}
    for q in (1, 95, 100):
        for s in (0, 1, 2):
            rng = np.random.default_rng(100 * q + s)
            imgs = []
            for k, (w, h) in enumerate(SIZES):
                imgs.append(rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
                imgs.append(_smooth(h, w, k + s))
            out[(q, s)] = imgs
    out[(95, 0)].append(np.random.default_rng(8).integers(0, 256, (8, 8, 3)).astype(np.uint8))
    out[(100, 0)].append(np.random.default_rng(0).integers(0, 256, (40, 40, 3), dtype=np.uint8))
    return out


def pil_bytes(rgb, quality=95, subsampling=2):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(b, "JPEG", quality=int(quality), subsampling=int(subsampling))
    return b.getvalue()


def canvas(images):
    """Images of unequal sizes as one source tensor: (u8 [n, hmax, wmax, 3], rects [(slot, 0, 0, w, h)])."""
    hmax, wmax = max(im.shape[0] for im in images), max(im.shape[1] for im in images)
    src = np.zeros((len(images), hmax, wmax, 3), dtype=np.uint8)
    for i, im in enumerate(images):
        src[i, :im.shape[0], :im.shape[1]] = im
    return src, [(i, 0, 0, im.shape[1], im.shape[0]) for i, im in enumerate(images)]


def host_write(lib, coeffs, desc, cap=None):
    """avcer_jpeg_write_batch, the oracle: (files as a list of bytes, offsets, status per file = its reason, bytes needed)."""
    d = desc.copy()
    out = np.zeros(623 * len(d) + 420 * (coeffs.size // 64), dtype=np.uint8)
    offsets, need = jpeg.write_batch(lib, np.ascontiguousarray(coeffs.reshape(-1)), d, out, 1, cap_bytes=cap)
    assert ((d["status"] == jpeg.OK) == (d["reason"] == 0)).all()
    return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(len(d))], offsets, d["reason"].astype(np.int32), need


# ------------------------------------------------------------------------------------------------ what a scan holds
def _code_lengths(dht):
    """{symbol: code length} of one DHT segment (marker and length included, as in the file)."""
    bits, vals = dht[5:21], dht[21:]
    out, p = {}, 0
    for l, c in enumerate(bits, 1):
        for _ in range(c):
            out[vals[p]] = l
            p += 1
    return out


def scan_stats(blob, coeffs, d):
    """(bits of the scan before the last byte is filled, ZRL symbols in it) of the file `blob` that was written from descriptor `d`:
    the blocks walked in scan order, code lengths read from the file's own DHT segments."""
    at = 177
    tabs = []
    for size in (33, 183, 33, 183):  # DC 0, AC 0, DC 1, AC 1
        tabs.append(_code_lengths(blob[at:at + size]))
        at += size
    hs, vs, mx, my = int(d["hs"]), int(d["vs"]), int(d["bw"][1]), int(d["bh"][1])
    blocks = coeffs.reshape(-1, 64)[int(d["coef_block"]):int(d["coef_block"] + d["n_blocks"])].astype(np.int64)
    base = [0, int(d["bw"][0] * d["bh"][0]), int(d["bw"][0] * d["bh"][0] + mx * my)]
    pred, bits, zrl = [0, 0, 0], 0, 0
    for y in range(my):
        for x in range(mx):
            for c in range(3):
                for v in range(vs if c == 0 else 1):
                    for u in range(hs if c == 0 else 1):
                        ch, cv = (hs, vs) if c == 0 else (1, 1)
                        blk = blocks[base[c] + (y * cv + v) * int(d["bw"][c]) + x * ch + u]
                        nb = int(abs(int(blk[0]) - pred[c])).bit_length()
                        pred[c] = int(blk[0])
                        bits += tabs[2 * (c > 0)][nb] + nb
                        run = 0
                        for k in range(1, 64):
                            t = int(blk[NATURAL[k]])
                            if t == 0:
                                run += 1
                                continue
                            zrl += run >> 4
                            bits += (run >> 4) * tabs[2 * (c > 0) + 1][0xF0]
                            nb = abs(t).bit_length()
                            bits += tabs[2 * (c > 0) + 1][((run & 15) << 4) | nb] + nb
                            run = 0
                        if run:
                            bits += tabs[2 * (c > 0) + 1][0]
    return bits, zrl


def stuffed_bytes(blob):
    scan = blob[623:-2]
    return sum(1 for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] == 0)
