"""A double-precision MPEG-1 I/P encoder and an exhaustive model of the motion search: the yardsticks the integer encoder
(espflix_amd/csrc/enc_core.h, k_encode.hip) is measured against (tests/test_encode_yardstick.py, tests/test_gpu_encode.py).
Not product code, numpy only, and nothing of enc_core.h: the rules are restated from their description.

  encode()     closed loop on its own reconstruction, no bitstream: orthonormal float64 DCT, the MPEG-1 quantisation rules
               with the default intra matrix (intra DC the rounded mean, intra AC rounded to nearest, non-intra truncated,
               |level| <= 255), the standard's dequantisation (oddification, +-2047), a float IDCT rounded to integers, the
               decoder's clamp to 0..248 and its four-case half-pel prediction.
  decisions()  (intra, h, v) of every macroblock of a P picture: every legal integer vector within +-search ordered by
               cost (the SAD, the zero vector's less 128), then |dx| + |dy|, then raster index; then the winner against
               its 8 half-pel neighbours (the centre wins ties, then the lowest neighbour in raster order); intra when
               the luma's absolute deviation from its rounded mean, plus 512, is below the winner's SAD."""
import numpy as np

import encode_model as E

W, H, CW, CH = 352, 192, 176, 96
MBX, MBY = W // 16, H // 16
PIC = W * H + 2 * CW * CH

# ISO 11172-2 2.4.3.2: the default intra quantiser matrix, raster order
INTRA_Q = np.array([[8, 16, 19, 22, 26, 27, 29, 34],
                    [16, 16, 22, 24, 27, 29, 34, 37],
                    [19, 22, 26, 27, 29, 34, 34, 38],
                    [22, 22, 26, 27, 29, 34, 37, 40],
                    [22, 26, 27, 29, 32, 35, 40, 48],
                    [26, 27, 29, 32, 35, 40, 48, 58],
                    [26, 27, 29, 34, 38, 46, 56, 69],
                    [27, 29, 35, 38, 46, 56, 69, 83]], dtype=np.float64)

# Orthonormal 8-point DCT-II: DCT[u, x] = c(u) cos((2x + 1) u pi / 16), c(0) = sqrt(1 / 8), c(u) = 1 / 2
DCT = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)]
                for u in range(8)])


def dct2(blocks):
    """Standard 2-D DCT of (..., 8, 8) blocks (ISO 11172-2 annex A units: a flat block of value m has DC 8 m)."""
    return DCT @ np.asarray(blocks, dtype=np.float64) @ DCT.T


def idct2(coef):
    return DCT.T @ np.asarray(coef, dtype=np.float64) @ DCT


def planes(pic):
    """One I420 picture -> (Y, Cb, Cr) int32 planes."""
    pic = np.asarray(pic).reshape(PIC)
    y = pic[:W * H].reshape(H, W).astype(np.int32)
    cb = pic[W * H:W * H + CW * CH].reshape(CH, CW).astype(np.int32)
    cr = pic[W * H + CW * CH:].reshape(CH, CW).astype(np.int32)
    return y, cb, cr


def to_blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def from_blocks(blocks):
    by, bx = blocks.shape[:2]
    return blocks.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


# -- quantisation -----------------------------------------------------------------------------------------------------

def quantise(F, intra, q):
    """Levels of standard-unit coefficients F (..., 8, 8), raster order.  intra: bool, broadcast over the blocks."""
    F = np.asarray(F, dtype=np.float64)
    intra = np.broadcast_to(np.asarray(intra, dtype=bool)[..., None, None], F.shape)
    a = np.abs(F)
    lev_i = np.floor(8 * a / (q * INTRA_Q) + 0.5)
    lev_n = np.floor(8 * a / (16.0 * q))
    lev = np.minimum(np.where(intra, lev_i, lev_n), 255) * np.sign(F)
    dc = np.clip(np.floor(F[..., 0, 0] / 8 + 0.5), 0, 255)
    lev[..., 0, 0] = np.where(intra[..., 0, 0], dc, lev[..., 0, 0])
    return lev.astype(np.int64)


def dequantise(lev, intra, q):
    """ISO 11172-2 2.4.4.1 / 2.4.4.2: coefficients of the levels, oddified towards zero and clipped to +-2047."""
    lev = np.asarray(lev, dtype=np.int64)
    intra = np.broadcast_to(np.asarray(intra, dtype=bool)[..., None, None], lev.shape)
    a = np.abs(lev)
    wq = (q * INTRA_Q).astype(np.int64)
    v = np.where(intra, (2 * a * wq) >> 4, ((2 * a + 1) * q * 16) >> 4)
    v = np.where((v & 1) == 0, v - 1, v)
    v = np.where(a == 0, 0, np.minimum(v, 2047)) * np.sign(lev)
    v[..., 0, 0] = np.where(intra[..., 0, 0], 8 * lev[..., 0, 0], v[..., 0, 0])
    return v


def code_plane(src, pred, intra_blocks, q):
    """Transform, quantise and reconstruct one plane: src / pred int planes, intra_blocks bool per 8 x 8 block (the
    prediction of an intra block is not used).  Returns the reconstruction."""
    intra_px = np.repeat(np.repeat(intra_blocks, 8, axis=0), 8, axis=1)
    pred = np.where(intra_px, 0, pred)
    F = dct2(to_blocks(src - pred))
    coef = dequantise(quantise(F, intra_blocks, q), intra_blocks, q)
    res = np.floor(idct2(coef) + 0.5).astype(np.int64)
    return np.clip(from_blocks(res) + pred, 0, 248).astype(np.int32)


# -- prediction -------------------------------------------------------------------------------------------------------

PAD = 18  # a margin of zeros around the reference planes: the integer stage shifts whole planes by up to 15 pels


def phase_planes(plane):
    """The four half-pel phases of a padded plane: P[hy][hx][y + PAD, x + PAD] predicts the pel at half-pel (2x + hx,
    2y + hy) -- the decoder's four cases."""
    a = np.pad(np.asarray(plane, dtype=np.int32), PAD + 1)[1:, 1:]  # PAD before, PAD + 1 after
    p00 = a[:-1, :-1]
    p10 = (a[:-1, :-1] + a[:-1, 1:] + 1) >> 1
    p01 = (a[:-1, :-1] + a[1:, :-1] + 1) >> 1
    p11 = (a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1] + a[1:, 1:] + 2) >> 2
    return ((p00, p10), (p01, p11))


def fetch(phases, px, py, size):
    """size x size prediction with its top-left at half-pel (px, py)."""
    y0, x0 = (py >> 1) + PAD, (px >> 1) + PAD
    return phases[py & 1][px & 1][y0:y0 + size, x0:x0 + size]


def axis_fits(mb, d, size):
    """Half-pel displacement d of macroblock index mb along an axis of `size` luma pels: the luma fetch (16 pels, 17 at a
    half-pel position) and the chroma fetch (8 pels, 9 at a half-pel position; chroma position = luma position >> 1)
    both stay inside the picture."""
    p = mb * 32 + d
    first, last = p >> 1, (p >> 1) + 15 + (p & 1)
    c = p >> 1
    cfirst, clast = c >> 1, (c >> 1) + 7 + (c & 1)
    return first >= 0 and last <= size - 1 and cfirst >= 0 and clast <= size // 2 - 1


def legal(mbx, mby, h, v):
    return axis_fits(mbx, h, W) and axis_fits(mby, v, H)


# -- search -----------------------------------------------------------------------------------------------------------

def search_picture(src_y, ref_y, R):
    """The search and mode rule on luma planes: (intra, h, v, sad) per macroblock, (12, 22) arrays; sad is the winner's
    SAD (before the intra decision zeroes the vector)."""
    src_y = np.asarray(src_y, dtype=np.int32)
    refp = np.pad(np.asarray(ref_y, dtype=np.int32), PAD)
    big = np.iinfo(np.int64).max
    best_cost = np.full((MBY, MBX), big, dtype=np.int64)
    best_dist = np.zeros((MBY, MBX), dtype=np.int64)
    best_dx = np.zeros((MBY, MBX), dtype=np.int64)
    best_dy = np.zeros((MBY, MBX), dtype=np.int64)
    okx = {dx: np.array([axis_fits(m, 2 * dx, W) for m in range(MBX)]) for dx in range(-R, R + 1)}
    oky = {dy: np.array([axis_fits(m, 2 * dy, H) for m in range(MBY)]) for dy in range(-R, R + 1)}
    for dy in range(-R, R + 1):          # raster order of the window: ties on cost and distance keep the earlier one
        for dx in range(-R, R + 1):
            ok = oky[dy][:, None] & okx[dx][None, :]
            if not ok.any():
                continue
            cand = refp[PAD + dy:PAD + dy + H, PAD + dx:PAD + dx + W]
            sad = np.abs(cand - src_y).reshape(MBY, 16, MBX, 16).sum(axis=(1, 3)).astype(np.int64)
            cost = np.maximum(sad - 128, 0) if dx == 0 and dy == 0 else sad
            dist = abs(dx) + abs(dy)
            better = ok & ((cost < best_cost) | ((cost == best_cost) & (dist < best_dist)))
            best_cost = np.where(better, cost, best_cost)
            best_dist = np.where(better, dist, best_dist)
            best_dx = np.where(better, dx, best_dx)
            best_dy = np.where(better, dy, best_dy)
    assert (best_cost < big).all()       # the zero vector is always legal
    phases = phase_planes(ref_y)
    intra = np.zeros((MBY, MBX), dtype=np.int64)
    hv = np.zeros((2, MBY, MBX), dtype=np.int64)
    sads = np.zeros((MBY, MBX), dtype=np.int64)
    for mby in range(MBY):
        for mbx in range(MBX):
            cur = src_y[mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16]
            ch, cv = 2 * int(best_dx[mby, mbx]), 2 * int(best_dy[mby, mbx])
            best = None
            for j in range(9) if R else (4,):
                h, v = ch + j % 3 - 1, cv + j // 3 - 1
                if not legal(mbx, mby, h, v):
                    continue
                sad = int(np.abs(fetch(phases, mbx * 32 + h, mby * 32 + v, 16) - cur).sum())
                cost = max(sad - 128, 0) if h == 0 and v == 0 else sad
                # (the zero vector is a half-pel candidate only as the centre: a neighbour of an integer winner is odd)
                key = (cost, 0 if j == 4 else 1 + j)
                if best is None or key < best[0]:
                    best = (key, h, v, sad)
            _, h, v, sad = best
            mean = (int(cur.sum()) + 128) >> 8
            dev = int(np.abs(cur - mean).sum())
            sads[mby, mbx] = sad
            if dev + 512 < sad:
                intra[mby, mbx] = 1
            else:
                hv[0, mby, mbx], hv[1, mby, mbx] = h, v
    return intra, hv[0], hv[1], sads


def decisions(src_picture, ref_picture, search):
    """(intra, h, v) per macroblock, (12, 22) arrays, of the I420 picture src_picture coded as a P picture from the I420
    reference ref_picture; h / v the half-pel luma vector, 0 where intra."""
    intra, h, v, _ = search_picture(planes(src_picture)[0], planes(ref_picture)[0], search)
    return intra, h, v


# -- the yardstick encoder ------------------------------------------------------------------------------------------------

def predict(ref_planes, intra, h, v):
    """Prediction planes of a P picture (zero where a macroblock is intra)."""
    out = [np.zeros((H, W), dtype=np.int32), np.zeros((CH, CW), dtype=np.int32), np.zeros((CH, CW), dtype=np.int32)]
    ph = [phase_planes(p) for p in ref_planes]
    for mby in range(MBY):
        for mbx in range(MBX):
            if intra[mby, mbx]:
                continue
            px, py = mbx * 32 + int(h[mby, mbx]), mby * 32 + int(v[mby, mbx])
            out[0][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16] = fetch(ph[0], px, py, 16)
            for c in (1, 2):
                out[c][mby * 8:mby * 8 + 8, mbx * 8:mbx * 8 + 8] = fetch(ph[c], px >> 1, py >> 1, 8)
    return out


def encode(pics, gop=12, qscale=8, search=7):
    """The yardstick's reconstruction (n, 101376) of the (n, 101376) I420 pictures: picture p is an I picture when
    p % gop == 0, else a P picture predicted from the yardstick's own reconstruction of picture p - 1."""
    pics = np.asarray(pics, dtype=np.uint8).reshape(-1, PIC)
    recon = np.empty_like(pics)
    ref = None
    for p, pic in enumerate(pics):
        src = planes(pic)
        if p % gop == 0:
            intra = np.ones((MBY, MBX), dtype=bool)
            pred = [np.zeros_like(s) for s in src]
        else:
            i, h, v, _ = search_picture(src[0], ref[0], search)
            intra = i.astype(bool)
            pred = predict(ref, intra, h, v)
        ref = [code_plane(src[0], pred[0], np.repeat(np.repeat(intra, 2, axis=0), 2, axis=1), qscale),
               code_plane(src[1], pred[1], intra, qscale), code_plane(src[2], pred[2], intra, qscale)]
        recon[p] = np.concatenate([r.reshape(-1) for r in ref]).astype(np.uint8)
    return recon


# -- helpers ----------------------------------------------------------------------------------------------------------

def luma_psnr_pictures(src, recon):
    """Luma PSNR of every picture, source values above 248 taken as 248 (the decoder's clamp), as E.luma_psnr does."""
    y0 = np.minimum(np.asarray(src).reshape(-1, PIC)[:, :W * H].astype(np.float64), 248)
    y1 = np.asarray(recon).reshape(-1, PIC)[:, :W * H].astype(np.float64)
    mse = np.maximum(((y0 - y1) ** 2).mean(axis=1), 1e-10)
    return 10 * np.log10(255.0 ** 2 / mse)


def psnr_by_type(src, recon, gop):
    """(mean luma PSNR of the I pictures, of the P pictures)."""
    ps = luma_psnr_pictures(src, recon)
    is_i = np.arange(len(ps)) % gop == 0
    return float(ps[is_i].mean()), float(ps[~is_i].mean()) if (~is_i).any() else float("nan")


BIG_STEPS = ((29, -27), (-31, 30), (17, 31), (-30, -31))


def big_motion(n):
    """E.moving with steps of 8.5 to 15.5 pels: at every search radius R <= 15 the best vectors lie on the window's edge,
    |h| and |v| reach 2 R + 1."""
    return E.moving(n, steps=BIG_STEPS)
