"""Plain numpy restatement of the f16x2 fragments of float32 tables (csrc/kde_kernels.hpp: h_piece, split2, split3s, f16x2_store_row;
csrc/kde_sweep_f16.inc: pack_rows_f16_kernel, kde_far_fix_kernel) and of what the five sweep kernels over them have to add up to.  Nothing
here needs a GPU or the library; tests/test_f16_restatement_cpu.py checks it against exact arithmetic, tests/test_f16_stages_gpu.py holds the
kernels against it stage by stage.

The pieces.  h_piece(x) = f16(x) rounded to nearest even, and 0 where |f16(x)| < 2^-14: no piece is ever an f16 subnormal (split2 below says from
which type the coordinate pieces are rounded on the device).
  split2(z)   z clamped to +-65504; a1 = h_piece(z), lo = h_piece((z - a1) 2^6), a2 = lo 2^-6, z^ = a1 + a2.
  split3s(x)  x clamped to +-65504 x 2^15; p1 = h_piece(x 2^-15), r = x - p1 2^15, p2 = h_piece(r 2^-5), r -= p2 2^5, p3 = h_piece(r 2^6).

The bounds that are TRUE (the code's comments used to promise |z - z^| <= 2^-22 |z| and a norm residual <= 2^-33 |x| without the floors):
  |z - z^| <= max(2^-22 |z|, 2^-20)   for |z| <= 65504.
      Proof.  Let a1 = h_piece(z), r = z - a1 (exact in double) and |z| in [2^e, 2^(e+1)).
      (A) a1 is a normal f16, the nearest to z (the source's float step moves z by <= 2^(e-23) first and changes a1 only next to a midpoint):
          |r| <= 2^(e-11) (1 + 2^-12) - half an f16 ulp of the binade, plus that step.  lo = h_piece(r 2^6); the scaling is exact.
          If lo is a normal f16, a2 is the f16 nearest to r.  For |r| < 2^(e-11), r lies in a binade no higher than [2^(e-12), 2^(e-11)), whose
          half ulp is 2^(e-23): |r - a2| <= 2^(e-23).  For |r| in [2^(e-11), 2^(e-11) (1 + 2^-12)] (the exact tie r = 2^(e-11), or the float
          step's excess over it) a2 = 2^(e-11) and |r - a2| <= 2^(e-23) again.  With the float step of r 2^6 itself (<= 2^-24 |r|) the error is
          <= 2^(e-23) (1 + 2^-11) <= 2^-22 |z|.
          If lo is flushed, |f16(r 2^6)| < 2^-14, so |r| < 2^-20 and the error is |r| itself: < 2^-20, ABSOLUTE.
      (B) the f16 nearest to z is below 2^-14: a1 = 0, r = z, |z| < 2^-14.  A normal lo holds z with 11 bits, error <= 2^-11 |z| (1 + 2^-13) <
          2^-25; a flushed lo means |z| < 2^-20 and the error is |z|.  Both lie under the floor.
      So the relative bound 2^-22 |z| holds exactly where the low piece is not flushed, and the error is the absolute |z - a1| < 2^-20 wherever
      |z - a1| < 2^-20, which values next to an f16 meet up to |z| ~ 4.
      (Observed worst over 2 10^5 normal draws per scale 1e-6 ... 6e4: 0.9995 x 2^-20.)
  |x - (2^15 p1 + 2^5 p2 + 2^-6 p3)| <= max(2^-33 |x|, 2^-20)   for float x, |x| <= 65504 x 2^15.
      Proof.  Every subtraction of split3s is exact in float (the subtrahend is the f16 rounding of the minuend's leading bits).  A piece is
      flushed only when the residual in front of it is below 2^-14 of its scale: p1 below |x| = 2, p2 below |r| = 2^-9, p3 below |r| = 2^-20.  With
      no flush the three 11-bit pieces leave <= 2^-11 2^-11 2^-11 |x| = 2^-33 |x|; a flushed p1 or p2 hands its whole residual to the next
      piece, which is then relative to a smaller number; a flushed p3 leaves |r| < 2^-20.  (Observed worst for |x| up to 50: 9.5e-7 = 0.9995 x 2^-20.)
  Scaled roles.  The slots a1 2^-6 and a2 (= lo 2^-6) go through h_piece as well: a1 2^-6 is stored as 0 for |a1| < 2^-8, a2 for |a2| < 2^-14.
      The slot products of a coordinate therefore sum to z^_t z^_q (spd = 4) or z^_t z^_q - a2 b2 (spd = 3) EXACTLY where no scaled role is
      flushed, and fall short by the products of the flushed roles otherwise: |a1 b2| < 2^-8 2^-11 |b| and |a2 b2| < 2^-14 2^-11 max(|a|, |b|), at most
      2^-19 (|z^_t| + |z^_q|) (1 + 2^-6) per coordinate.  The sweeps and this restatement's exponents use the slots as they are; kde_far_fix_kernel
      decodes z^ = slot 0 + slot 2 2^-6, which no flush of a scaled role touches.

The layout.  Slot s of a row lives in MFMA block s / 32, lane group (s % 32) / 8, element s % 8; fragment arrays are [tile][NB][64 lanes][8]
with lane = 16 group + row % 16.  slot_map(dm, NB, query) names every slot.
"""
import math
from fractions import Fraction

import numpy as np

H_MAX = 65504.0
H_C = (32768.0, 32.0, 0.015625)            # PBN_H_C1, C2, C3
H_LO = 64.0
X_MAX = np.float32(H_MAX * 32768.0)
PAD_NORM = -1e30
F16_MIN_NORMAL = 2.0 ** -14
MAX_DM = 32                                 # kde_prepare: max_dm of the f16x2 path; launch_sweep_f16 serves NB = f16x2_blocks(dm) <= 7


def ceil_div(a, b):
    return -(-a // b)


def blocks(dm):                             # f16x2_blocks
    return (3 * dm + 3 + 31) // 32


def spd(dm):                                # f16x2_spd
    return 4 if 4 * dm + 3 <= 32 * blocks(dm) else 3


def w32_applies(dm, NB):                    # f16x2_w32 with PBN_F32_W32 on
    return NB in (1, 2) and spd(dm) * dm + 6 <= 32 * NB


def w32p_applies(dm, NB):                   # f16x2_w32p
    return NB == 1 and spd(dm) * dm + 6 <= 32


# ---- pieces -------------------------------------------------------------------------------------------------------------------------------
def h_piece(x):
    """f16 of x (one rounding to nearest even from x's own type, float32 or float64), subnormals flushed to +0."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    return np.where(np.abs(h.astype(np.float32)) < np.float32(F16_MIN_NORMAL), np.float16(0.0), h)


def split2(z, by_float=False):
    """z (float64) -> hi = a1, lo = a2 2^6 (float16), the represented value a1 + a2 (float64), clamped flags.
    The source reads hi = h_piece((float)z): double -> float -> half.  The compiled kernel rounds ONCE, double -> half (the two conversions are
    contracted; seen on the device at z = w x one double below an f16 midpoint, w = 1 - 2^-53, which the float step would have put ON the
    midpoint) - that is what this restates; by_float=True gives the source's order.  The two differ only where z lies within 2^-24 |z| of an f16
    midpoint, never for a z that is a float itself, and every bound here holds for both (test_f16_restatement_cpu.py checks both)."""
    z = np.asarray(z, dtype=np.float64)
    clamped = ~(np.abs(z) <= H_MAX)
    z = np.where(z > H_MAX, H_MAX, np.where(z < -H_MAX, -H_MAX, z))
    z = np.where(np.isnan(z), 0.0, z)
    hi = h_piece(z.astype(np.float32) if by_float else z)
    r = z - hi.astype(np.float64)
    lo = h_piece((r * H_LO).astype(np.float32) if by_float else r * H_LO)
    return hi, lo, hi.astype(np.float64) + lo.astype(np.float64) * (1.0 / H_LO), clamped


def split3s(x):
    """x (float32) -> the three float16 pieces of 2^15 p1 + 2^5 p2 + 2^-6 p3, in float32 arithmetic."""
    x = np.asarray(x, dtype=np.float32)
    x = np.where(x > X_MAX, X_MAX, np.where(x < -X_MAX, -X_MAX, x)).astype(np.float32)
    x = np.where(np.isnan(x), -X_MAX, x).astype(np.float32)
    c1, c2, c3 = (np.float32(c) for c in H_C)
    p1 = h_piece(x * np.float32(1.0 / H_C[0]))
    r = (x - p1.astype(np.float32) * c1).astype(np.float32)
    p2 = h_piece(r * np.float32(1.0 / H_C[1]))
    r = (r - p2.astype(np.float32) * c2).astype(np.float32)
    p3 = h_piece(r * np.float32(1.0 / H_C[2]))
    return p1, p2, p3


def join3(p1, p2, p3):
    """The value three norm pieces stand for against the constants, exact in float64."""
    return p1.astype(np.float64) * H_C[0] + p2.astype(np.float64) * H_C[1] + p3.astype(np.float64) * H_C[2]


def scaled(h):
    """h 2^-6 as a slot holds it: h_piece((float)h / 64)."""
    return h_piece(h.astype(np.float32) * np.float32(1.0 / H_LO))


def _fma(a, b, c):
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))             # correctly rounded


def half_norm(zr):
    """float32(-1/2 sum_k zr_k^2) with the sum formed as the kernels form it: nrm = fma(zr_k, zr_k, nrm), k ascending, in double."""
    zr = np.asarray(zr, dtype=np.float64)
    out = np.empty(zr.shape[0], dtype=np.float32)
    for i, row in enumerate(zr):
        nrm = 0.0
        for v in row:
            nrm = _fma(float(v), float(v), nrm)
        out[i] = np.float32(-0.5 * nrm)
    return out


# ---- the slot map -------------------------------------------------------------------------------------------------------------------------
def slot_map(dm, NB, query):
    """Per slot of the main contraction (32 NB of them) a tuple: ("hi", k) a1 of coordinate k, ("hi_s", k) a1 2^-6, ("lo", k) a2 2^6, ("lo_u", k)
    a2, ("norm", t) the t-th norm piece (training), ("const", t) the constant 2^15, 2^5, 2^-6, ("zero",).  Roles of f16x2_store_row: training
    (a1, a1 2^-6, a2 2^6, a2), query (b1, b2 2^6, b1 2^-6, b2); behind them the norm pieces against the constants; the last three slots of the
    training side carry the constants again when they are free (spd dm + 6 <= 32 NB: the W32 forms' query offsets meet them)."""
    s_ = spd(dm)
    roles = ("hi", "lo", "hi_s", "lo_u") if query else ("hi", "hi_s", "lo", "lo_u")
    out = []
    for s in range(32 * NB):
        if s < s_ * dm:
            out.append((roles[s % s_], s // s_))
            continue
        t = s - s_ * dm
        if t < 3:
            out.append(("const", t) if query else ("norm", t))
        elif not query and s >= 32 * NB - 3 and s_ * dm + 6 <= 32 * NB:
            out.append(("const", s - (32 * NB - 3)))
        else:
            out.append(("zero",))
    return out


def extra_map(query):
    """The CKDE block (one more 32-slot MFMA): the extra coordinate in three products, its norm against the constants, and the constants
    against the query's norm pieces in the rewritable slots 8..10."""
    z = [("zero",)] * 32
    if query:
        z[0:6] = [("hi", 0), ("lo", 0), ("hi_s", 0), ("const", 0), ("const", 1), ("const", 2)]
        z[8:11] = [("norm", 0), ("norm", 1), ("norm", 2)]
    else:
        z[0:6] = [("hi", 0), ("hi_s", 0), ("lo", 0), ("norm", 0), ("norm", 1), ("norm", 2)]
        z[8:11] = [("const", 0), ("const", 1), ("const", 2)]
    return z


def fill_slots(smap, hi, lo, norm_pieces):
    """Slot vectors [rows][len(smap)] (float16) of rows with pieces hi, lo [rows][dims] and norm pieces (p1, p2, p3) each [rows]."""
    n = hi.shape[0]
    out = np.zeros((n, len(smap)), dtype=np.float16)
    hi_s, lo_u = scaled(hi), scaled(lo)
    src = {"hi": hi, "lo": lo, "hi_s": hi_s, "lo_u": lo_u}
    for s, what in enumerate(smap):
        if what[0] in src:
            out[:, s] = src[what[0]][:, what[1]]
        elif what[0] == "norm":
            out[:, s] = norm_pieces[what[1]]
        elif what[0] == "const":
            out[:, s] = np.float16(H_C[what[1]])
    return out


def pack_rows(z, n_valid, dm, NB, query, cond):
    """What pack_rows_f16_kernel writes for whitened rows z [n_valid][d] (float64, d = dm + cond): dict(slots [16 tiles][32 NB] float16, npack
    (query: float32 per row), xslots [..][32], xnorm (query, cond), far (query flags), zr [..][d] the represented values); padding rows of the
    last tile included (coordinates 0; norm 0 on the query side, PBN_PAD_NORM - clamped by split3s - on the training side)."""
    npad = ceil_div(n_valid, 16) * 16
    d = dm + (1 if cond else 0)
    zz = np.zeros((npad, d))
    zz[:n_valid] = z
    hi, lo, zr, cl = split2(zz)
    nv = half_norm(zr[:, :dm])
    nv[n_valid:] = np.float32(0.0 if query else PAD_NORM)
    out = dict(zr=zr, slots=fill_slots(slot_map(dm, NB, query), hi[:, :dm], lo[:, :dm], split3s(nv)))
    far = cl[:, :dm].any(axis=1)
    if query:
        out["npack"] = nv
    if cond:
        hn = (-0.5 * zr[:, dm] * zr[:, dm]).astype(np.float32)
        out["xslots"] = fill_slots(extra_map(query), hi[:, dm:], lo[:, dm:], split3s(hn))
        far = far | cl[:, dm]
        if query:
            out["xnorm"] = hn
    if query:
        far[n_valid:] = False
        out["far"] = far.astype(np.uint8)
    return out


# ---- decoders -----------------------------------------------------------------------------------------------------------------------------
def decode_main(frag_u16, ntiles, NB):
    """[ntiles][NB][64][8] f16 bit patterns -> slot vectors [16 ntiles][32 NB] (float16): slot s = 32 block + 8 group + element, lane = 16 group + row."""
    a = np.asarray(frag_u16, dtype=np.uint16).reshape(ntiles, NB, 4, 16, 8)
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2, 4)).reshape(ntiles * 16, NB * 32).view(np.float16)


def decode_extra(frag_u16, ntiles):
    return decode_main(frag_u16, ntiles, 1)


def bits(h):
    return np.ascontiguousarray(h, dtype=np.float16).view(np.uint16)


def decoded_pieces(slots, smap):
    """hi, lo [rows][dims] and the three norm pieces (None on a side that carries constants) of slot vectors."""
    dims = 1 + max((w[1] for w in smap if w[0] == "hi"), default=-1)
    hi = np.zeros((slots.shape[0], dims), dtype=np.float16)
    lo = np.zeros_like(hi)
    norm = [None, None, None]
    for s, what in enumerate(smap):
        if what[0] == "hi":
            hi[:, what[1]] = slots[:, s]
        elif what[0] == "lo":
            lo[:, what[1]] = slots[:, s]
        elif what[0] == "norm":
            norm[what[1]] = slots[:, s]
    return hi, lo, norm


def represented(hi, lo):
    return hi.astype(np.float64) + lo.astype(np.float64) * (1.0 / H_LO)


def consistent_slots(slots, smap):
    """The slot vectors that follow from the rows' OWN decoded (hi, lo, norm pieces): every other slot is a function of those."""
    hi, lo, norm = decoded_pieces(slots, smap)
    return fill_slots(smap, hi, lo, norm)


# ---- reference exponents and partials -----------------------------------------------------------------------------------------------------
def split_error_bound(z):
    return np.maximum(2.0 ** -22 * np.abs(z), 2.0 ** -20)


def norm_error_bound(x):
    return np.maximum(2.0 ** -33 * np.abs(x), 2.0 ** -20)


class Pairs:
    """Exponents of every (training row, query) pair from decoded operands, in float64: e = sum_s A[s] B[s] + off_q.  Products of two f16
    values are exact in float64; `mag` = sum |terms| + |off| and `nnz` = number of nonzero products carry the error model of the caller."""

    def __init__(self, A, B, off):
        A64, B64 = A.astype(np.float64), B.astype(np.float64)
        self.e = A64 @ B64.T + off[None, :]
        self.mag = np.abs(A64) @ np.abs(B64).T
        self.nnz = (A64 != 0).astype(np.float64) @ (B64 != 0).astype(np.float64).T

    def add(self, other_e, other_mag, other_nnz):
        self.e = self.e + other_e
        self.mag = self.mag + other_mag
        self.nnz = self.nnz + other_nnz


def log2_sum(e, axis=0):
    m = e.max(axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (m + np.log2(np.exp2(e - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def split_ranges(ntiles, tps, N):
    """Training rows [r0, r1) of every split (padding rows left out)."""
    out = []
    for t0 in range(0, ntiles, tps):
        out.append((t0 * 16, min(min(t0 + tps, ntiles) * 16, N)))
    return out


def merge_partials(part):
    """What kde_finish_kernel merges: per query log2 sum_splits s 2^m from part [nsplit][rows][2] -> [rows] (float64, stable)."""
    m, s = part[:, :, 0], part[:, :, 1]
    top = m.max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return top + np.log2((s * np.exp2(m - top[None, :])).sum(axis=0))
