"""CPU tier: tests/f16_restatement.py (the numpy restatement of the f16x2 fragments of float32 tables) against exact arithmetic.
  * for every dm the f16x2 path serves (1 ... 32: kde_prepare's max_dm; launch_sweep_f16 instantiates NB = f16x2_blocks(dm) up to 7), on both
    sides, with and without the CKDE block: no slot is used twice, none lies beyond 32 NB, every piece has its slot;
  * the slot products of the restated layout, in fractions.Fraction: sum_s A[s] B[s] = z^_t . z^_q - 1/2 |z^_t|^2 (the norm as its three pieces
    stand for it) exactly at spd = 4 and minus sum_k a2 b2 at spd = 3, where no scaled role is flushed; where one is, the deficit is the
    flushed products and stays inside 2^-19 (|z^_t| + |z^_q|) (1 + 2^-6) per coordinate;
  * the three norm pieces against the constants give back the clamped float norm within max(2^-33 |x|, 2^-20);
  * |z - z^| <= max(2^-22 |z|, 2^-20) over 2 10^5 normal draws at each of the scales 1e-6 ... 6e4 - and the pure relative bounds the code's
    comments used to state do NOT hold there (so the floors are needed, not slack).
"""
from fractions import Fraction

import numpy as np
import pytest

import f16_restatement as fr

SCALES = (1e-6, 1e-4, 3e-3, 0.05, 1.0, 4.0, 50.0, 3e3, 6e4)
DRAWS = 200_000


def _frac_rows(a):
    return [[Fraction(float(v)) for v in row] for row in a]


@pytest.mark.parametrize("dm", range(1, fr.MAX_DM + 1))
def test_slot_map_uses_every_slot_once(dm):
    NB, s = fr.blocks(dm), fr.spd(dm)
    assert 1 <= NB <= 7 and s in (3, 4)
    assert s * dm + 3 <= 32 * NB, "coordinates and norm fit the blocks"
    assert (s == 4) == (4 * dm + 3 <= 32 * NB)
    for query in (False, True):
        smap = fr.slot_map(dm, NB, query)
        assert len(smap) == 32 * NB
        used = [w for w in smap if w[0] != "zero"]
        assert len(set(used)) == len(used), "a slot named twice"
        want = {(r, k) for k in range(dm) for r in (("hi", "lo", "hi_s", "lo_u")[:s] if query else ("hi", "hi_s", "lo", "lo_u")[:s])}
        # three products: the query side has (b1, b2 2^6, b1 2^-6), the training side (a1, a1 2^-6, a2 2^6)
        coords = {w for w in used if w[0] in ("hi", "lo", "hi_s", "lo_u")}
        assert coords == want
        tail = [w for w in used if w not in coords]
        if query:
            assert tail == [("const", 0), ("const", 1), ("const", 2)]
        else:
            free = s * dm + 6 <= 32 * NB
            assert tail == [("norm", 0), ("norm", 1), ("norm", 2)] + ([("const", 0), ("const", 1), ("const", 2)] if free else [])
            if free:
                assert smap[-3:] == [("const", 0), ("const", 1), ("const", 2)]
            assert fr.w32_applies(dm, NB) == (free and NB <= 2)
    # the roles pair up: slot by slot the product of the two sides is a1 b1, a1 b2, a2 b1 (, a2 b2)
    pair = {("hi", "hi"), ("hi_s", "lo"), ("lo", "hi_s"), ("lo_u", "lo_u"), ("norm", "const")}
    for a, b in zip(fr.slot_map(dm, NB, False), fr.slot_map(dm, NB, True)):
        if a[0] != "zero" and b[0] != "zero":
            assert (a[0], b[0]) in pair and a[1] == b[1]
        else:
            assert b[0] == "zero" or a[0] == "zero"


def test_w32_dimensions_are_the_ones_the_launcher_names():
    got = [d for d in range(1, 33) if fr.w32_applies(d, fr.blocks(d))]
    assert got == [1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 16, 17, 18, 19], got   # d = 7 (31 slots), 9, 15 and 20 leave no three free slots
    assert [d for d in range(1, 33) if fr.w32p_applies(d, fr.blocks(d))] == [1, 2, 3, 4, 5, 6, 8]


def test_extra_block_pairs_up():
    t, q = fr.extra_map(False), fr.extra_map(True)
    pair = {("hi", "hi"), ("hi_s", "lo"), ("lo", "hi_s"), ("norm", "const"), ("const", "norm")}
    live = [(a, b) for a, b in zip(t, q) if a[0] != "zero" or b[0] != "zero"]
    assert len(live) == 9 and all((a[0], b[0]) in pair for a, b in live)
    assert [i for i, w in enumerate(q) if w[0] == "norm"] == [8, 9, 10]


@pytest.mark.parametrize("dm", range(1, fr.MAX_DM + 1))
def test_slot_products_sum_exactly(dm):
    rng = np.random.default_rng(100 + dm)
    NB, s = fr.blocks(dm), fr.spd(dm)
    n = 6
    # z = a1 + a2 built from its pieces: |a1| in [8, 400] (a1 2^-6 >= 2^-8 is no subnormal), |a2| in [1/16, 1/2) ulp(a1) >= 2^-11: no scaled role is flushed
    def draw():
        a1 = rng.uniform(8.0, 400.0, size=(n, dm)).astype(np.float16).astype(np.float64)
        ulp = 2.0 ** (np.floor(np.log2(a1)) - 10)
        a2 = (ulp * rng.uniform(1 / 16, 0.49, size=(n, dm))).astype(np.float16).astype(np.float64)
        return (a1 + a2 * rng.choice([-1.0, 1.0], size=(n, dm))) * rng.choice([-1.0, 1.0], size=(n, dm))

    zt, zq = draw(), draw()
    zt[0, 0] = 24.0                                                   # an exact f16: a2 = 0
    T, Q = fr.pack_rows(zt, n, dm, NB, False, False), fr.pack_rows(zq, n, dm, NB, True, False)
    hi_t, lo_t, _ = fr.decoded_pieces(T["slots"], fr.slot_map(dm, NB, False))
    hi_q, lo_q, _ = fr.decoded_pieces(Q["slots"], fr.slot_map(dm, NB, True))
    for h, l in ((hi_t, lo_t), (hi_q, lo_q)):
        assert np.all(np.abs(h[:n].astype(float)) >= 2.0 ** -8)
        a2 = np.abs(l[:n].astype(float)) / 64
        assert np.all((a2 == 0) | (a2 >= 2.0 ** -14)), "the draw must not flush a scaled role"
    A, B = _frac_rows(T["slots"][:n]), _frac_rows(Q["slots"][:n])
    ZT, ZQ = _frac_rows(T["zr"][:n]), _frac_rows(Q["zr"][:n])
    a2t, b2q = _frac_rows(lo_t[:n].astype(np.float64) / 64), _frac_rows(lo_q[:n].astype(np.float64) / 64)
    _, _, norm = fr.decoded_pieces(T["slots"], fr.slot_map(dm, NB, False))
    nt = fr.join3(*norm)
    for i in range(n):
        for j in range(n):
            got = sum(a * b for a, b in zip(A[i], B[j]))
            want = sum(x * y for x, y in zip(ZT[i], ZQ[j])) + Fraction(float(nt[i]))
            if s == 3:
                want -= sum(x * y for x, y in zip(a2t[i], b2q[j]))
            assert got == want, (dm, s, i, j, float(got - want))


def test_flushed_roles_leave_a_bounded_deficit():
    rng = np.random.default_rng(7)
    dm, n = 5, 40
    NB = fr.blocks(dm)
    zt = rng.normal(size=(n, dm)) * 10.0 ** rng.uniform(-5, 1.5, size=(n, dm))
    zq = rng.normal(size=(n, dm)) * 10.0 ** rng.uniform(-5, 1.5, size=(n, dm))
    T, Q = fr.pack_rows(zt, n, dm, NB, False, False), fr.pack_rows(zq, n, dm, NB, True, False)
    nslots = fr.spd(dm) * dm
    dot = T["slots"][:n, :nslots].astype(np.float64) @ Q["slots"][:n, :nslots].astype(np.float64).T
    want = T["zr"][:n] @ Q["zr"][:n].T
    bound = 2.0 ** -19 * (1 + 2.0 ** -6) * (np.abs(T["zr"][:n]).sum(axis=1)[:, None] + np.abs(Q["zr"][:n]).sum(axis=1)[None, :])
    slack = 64 * 2.0 ** -53 * (np.abs(T["zr"][:n]) @ np.abs(Q["zr"][:n]).T)
    assert np.any(dot != want), "the draw reaches the flushed roles"
    assert np.all(np.abs(dot - want) <= bound + slack)


@pytest.mark.parametrize("by_float", [False, True])
@pytest.mark.parametrize("scale", SCALES)
def test_split2_bound(scale, by_float):
    rng = np.random.default_rng(int(1e6 * np.log10(scale * 1e7)))
    z = rng.normal(size=DRAWS) * scale
    z = z[np.abs(z) <= fr.H_MAX]
    hi, lo, zr, cl = fr.split2(z, by_float)
    assert not cl.any()
    err = np.abs(z - zr)
    assert np.all(err <= fr.split_error_bound(z)), float((err / fr.split_error_bound(z)).max())
    assert np.all((hi == 0) | (np.abs(hi.astype(np.float64)) >= 2.0 ** -14)) and np.all((lo == 0) | (np.abs(lo.astype(np.float64)) >= 2.0 ** -14))
    assert np.all(err < 2.0 ** -20 * 1.0000001) or scale >= 4.0
    if scale == 1.0:
        rel = (err / np.abs(z)).max()
        assert rel > 2.0 ** -22, "the pure relative bound of the old comments fails at |z| ~ 1: the floor is needed"
        assert err.max() > 0.99 * 2.0 ** -20


def test_split2_clamps_and_flags():
    z = np.array([65504.0, -65504.0, 65504.0 * (1 + 2.0 ** -20), -65536.0, 1e30, np.inf, -np.inf, np.nan, 0.0, -0.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -20, 2.0 ** -21])
    hi, lo, zr, cl = fr.split2(z)
    assert cl.tolist() == [False, False, True, True, True, True, True, True, False, False, False, False, False, False]
    assert zr[:8].tolist() == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0, 65504.0, -65504.0, 0.0]
    assert zr[8:].tolist() == [0.0, 0.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -20, 0.0]      # 2^-15: a1 flushed, the low piece holds it; 2^-21: both flushed
    assert fr.bits(hi)[9] == 0 and fr.bits(lo)[9] == 0, "a flushed piece is +0"


@pytest.mark.parametrize("scale", SCALES + (1e7, 2e9))
def test_split3s_bound(scale):
    rng = np.random.default_rng(int(1e6 * np.log10(scale * 1e7)) + 1)
    x = (-np.abs(rng.normal(size=DRAWS)) * scale).astype(np.float32)
    x[:1000] = -x[:1000]
    p = fr.split3s(x)
    xc = np.clip(x.astype(np.float64), -float(fr.X_MAX), float(fr.X_MAX))
    err = np.abs(xc - fr.join3(*p))
    assert np.all(err <= fr.norm_error_bound(xc)), float((err / fr.norm_error_bound(xc)).max())
    for piece in p:
        assert np.all((piece == 0) | (np.abs(piece.astype(np.float64)) >= 2.0 ** -14)) and np.all(np.isfinite(piece.astype(np.float64)))
    if scale == 50.0:
        assert err.max() > 0.9 * 2.0 ** -20 and (err / np.abs(xc)).max() > 2.0 ** -33


def test_the_two_rounding_orders_differ_only_beside_a_midpoint():
    z = np.array([6.130859375 * (1 - 2.0 ** -53), 6.130859375, 1.0 + 2.0 ** -11 + 2.0 ** -40])      # one double below an f16 midpoint, on it, just above one
    one, two = fr.split2(z), fr.split2(z, by_float=True)
    assert one[0].tolist() == [6.12890625, 6.1328125, 1.0009765625] and two[0].tolist() == [6.1328125, 6.1328125, 1.0]
    for got in (one, two):
        assert np.all(np.abs(z - got[2]) <= fr.split_error_bound(z))
    x = (np.random.default_rng(3).normal(size=20000) * 37).astype(np.float32).astype(np.float64)
    assert all(np.array_equal(fr.bits(a), fr.bits(b)) for a, b in zip(fr.split2(x)[:2], fr.split2(x, True)[:2])), "floats: one order"


def test_padding_norm_and_nan():
    p = fr.split3s(np.array([fr.PAD_NORM, np.nan, 3e9, 0.0], dtype=np.float32))
    v = fr.join3(*p)
    assert v.tolist() == [-float(fr.X_MAX), -float(fr.X_MAX), float(fr.X_MAX), 0.0]


def test_half_norm_is_the_fma_chain():
    rng = np.random.default_rng(5)
    z = rng.normal(size=(50, 7)) * 30.0
    _, _, zr, _ = fr.split2(z)
    got = fr.half_norm(zr)
    for i in range(50):
        nrm = Fraction(0)
        for v in zr[i]:
            nrm = Fraction(float(Fraction(float(v)) ** 2 + nrm))       # one rounding per step
        assert got[i] == np.float32(-0.5 * float(nrm))


def test_decoders_invert_the_layout():
    rng = np.random.default_rng(9)
    dm, NB, n = 10, 2, 37
    P = fr.pack_rows(rng.normal(size=(n, dm + 1)) * 3, n, dm, NB, True, True)
    ntiles = fr.ceil_div(n, 16)
    # the layout as f16x2_store_row writes it: pack[(tile NB + mb) 64 + g 16 + idx][j] = slot(mb 32 + g 8 + j)
    frag = np.zeros((ntiles, NB, 64, 8), dtype=np.uint16)
    b = fr.bits(P["slots"])
    for r in range(ntiles * 16):
        for s in range(32 * NB):
            frag[r // 16, s // 32, ((s % 32) // 8) * 16 + r % 16, s % 8] = b[r, s]
    assert np.array_equal(fr.bits(fr.decode_main(frag.ravel(), ntiles, NB)), b)
    assert np.array_equal(fr.bits(fr.consistent_slots(P["slots"], fr.slot_map(dm, NB, True))), b)
    assert np.array_equal(fr.bits(fr.consistent_slots(P["xslots"], fr.extra_map(True))), fr.bits(P["xslots"]))
    assert P["far"].sum() == 0 and np.all(P["npack"][n:] == 0) and np.all(P["slots"][n:, : fr.spd(dm) * dm] == 0)


def test_reference_partials_merge_to_the_whole():
    rng = np.random.default_rng(11)
    dm, NB, N, n = 6, 1, 100, 9
    T = fr.pack_rows(rng.normal(size=(N, dm)), N, dm, NB, False, False)
    Q = fr.pack_rows(rng.normal(size=(n, dm)), n, dm, NB, True, False)
    pairs = fr.Pairs(T["slots"], Q["slots"], Q["npack"].astype(np.float64))
    assert np.all(pairs.e[N:] < -2.0 ** 30), "padding rows: the clamped PBN_PAD_NORM puts them 2^31 units down"
    want = -0.5 * ((T["zr"][:N, None, :] - Q["zr"][None, :n, :]) ** 2).sum(axis=2)
    assert np.abs(pairs.e[:N, :n] - want).max() < 2.0 ** -18        # the three norm pieces and the query's float norm: 2^-20 each at most here
    parts = np.stack([np.stack([np.zeros(16), np.exp2(fr.log2_sum(pairs.e[r0:r1]))], axis=1) for r0, r1 in fr.split_ranges(7, 3, N)])
    assert np.allclose(fr.merge_partials(parts)[:n], fr.log2_sum(pairs.e[:N])[:n], rtol=0, atol=1e-12)
