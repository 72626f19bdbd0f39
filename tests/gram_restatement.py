"""Plain Python restatement of the launch arithmetic of the contiguous Gram kernels (csrc/stats_kernels.hip gram_glds_kernel /
gram_glds_f32_kernel) in their two forms - the plain form behind pbn_table_sse (csrc/capi.hip table_gram -> launch_gram) and the segmented
form behind a score handle's moments (csrc/scoring.hip compute_stats_segments -> launch_gram_segments) - and the case lists of
tests/test_gram_shapes_gpu.py as functions of the device's CU count.  Shares nothing with the library: every constant is quoted with the
line it restates, and tests/test_gram_restatement_cpu.py checks without a device that the planned cases reach every state the GPU test
asserts at its end (required_states below).

A block's "ring state" is what decides which of the hand-counted s_waitcnt vmcnt(N) a wave executes: nfull, the whole chunks the block
moves by LDS-DMA (prologue fills min(2, nfull) stages; the steady loop runs while i + 4 < nfull; the drain takes the rest with waits that
depend on i + 2 < nfull), and whether a cut last chunk follows through registers."""
import numpy as np

# ---- the kernels' constants, each with the line it restates ------------------------------------------------------------------------------
GD_BLOCKS_PER_CU = 2     # stats_kernels.hip: constexpr int GD_BLOCKS_PER_CU = 2;
GD_STAGES = 2            # stats_kernels.hip: constexpr int GD_STAGES = 2;
GD_ROWS = 64             # stats_kernels.hip: constexpr int GD_ROWS = 64;    (double tables: 16 rows per wave)
GF_ROWS = 128            # stats_kernels.hip: constexpr int GF_ROWS = 128;   (float tables: 32 rows per wave)
REDUCE_ARITY = 16        # stats_kernels.hip launch_gram: while ((nblocks + stride - 1) / stride > 16) { ...; stride *= 16; }
SEG_ROWS = 4096          # scoring.hip seg_rows(): PBN_TUNE(MOMENT_SEG_ROWS, 4096)
PILOT_ROWS = 1024        # stats_kernels.hip pilot_mean_kernel: m = n < 1024 ? n : 1024
SUPER_BLOCKS = 16        # scoring.hip scoredata_create_impl: SB = sd->n <= 128 ? 16 : ...
PAIR_BLOCK = 32          # scoring.hip compute_stats_segments: nb = (n + 31) / 32;  capi.hip pbn_table_sse: const int B = 32
MAX_TABLE_BYTES = 128 << 20

NFULL_CLASSES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)   # 9 stands for >= 9
TAILS = ("none", "short", "long")                # no cut chunk / fewer rows than one wave's share of a chunk / at least that


def ceil_div(a, b):
    return -(-a // b)


def chunk_rows(es):
    """Rows of one block chunk for an element size in bytes."""
    return {8: GD_ROWS, 4: GF_ROWS}[es]


def nct_of(d):
    return ceil_div(d, 16)   # capi.hip table_gram: nct = (d + 15) / 16


# ---- plain form -----------------------------------------------------------------------------------------------------------------------------
def plain_blocks(n, num_cus):
    """capi.hip table_gram: nblocks = min(4 num_cus, max(1, ceil(n / 256))); rpb = ceil(max(n, 1) / nblocks) rounded up to 64;
    nblocks = max(1, ceil(n / rpb)).  Returns (nblocks, rpb)."""
    nblocks = min(4 * num_cus, max(1, ceil_div(n, 256)))
    rpb = ceil_div(max(n, 1), nblocks)
    rpb = (rpb + 63) // 64 * 64
    return max(1, ceil_div(n, rpb)), rpb


def plain_grid(nblocks, num_cus):
    """stats_kernels.hip launch_gram: if (!gather && a.num_cus > 0 && nblocks > GD_BLOCKS_PER_CU * a.num_cus) nblocks = GD_BLOCKS_PER_CU * a.num_cus;"""
    cap = GD_BLOCKS_PER_CU * num_cus
    return cap if nblocks > cap else nblocks


def reduce_levels(grid):
    """Launches of gram_reduce_kernel in launch_gram: one per level of the 16-ary tree over the grid's partials."""
    levels, stride = 1, 1
    while ceil_div(grid, stride) > REDUCE_ARITY:
        levels, stride = levels + 1, stride * REDUCE_ARITY
    return levels


def plain_block(b, B, n, C):
    """Block b of a grid of B on n rows (gram_glds_kernel, plain form): nchunks = ceil(n / C); first = b C; stride = B C;
    mine = b < nchunks ? (nchunks - 1 - b) / B + 1 : 0; partial_last = mine > 0 && first + (mine - 1) stride + C > n;
    nfull = mine - partial_last.  Returns (first, stride, mine, partial_last, nfull, tail rows of the cut chunk)."""
    nchunks = ceil_div(n, C)
    first, stride = b * C, B * C
    mine = (nchunks - 1 - b) // B + 1 if b < nchunks else 0
    partial_last = mine > 0 and first + (mine - 1) * stride + C > n
    nfull = mine - (1 if partial_last else 0)
    tail = n - (first + nfull * stride) if partial_last else 0
    return first, stride, mine, partial_last, nfull, tail


def piece_block(first, end, C):
    """A piece [first, end) of a segment (gram_glds_kernel, a.blk): stride = C; mine = ceil((end - first) / C); the same partial_last / nfull."""
    mine = ceil_div(end - first, C)
    partial_last = mine > 0 and first + (mine - 1) * C + C > end
    nfull = mine - (1 if partial_last else 0)
    tail = end - (first + nfull * C) if partial_last else 0
    return first, C, mine, partial_last, nfull, tail


def ring(nfull):
    """(trips of the steady loop `for (i = 0; i + 4 < nfull; i += 2)`, whole chunks it leaves to the drain loop)."""
    trips, i = 0, 0
    while i + 4 < nfull:
        trips, i = trips + 1, i + 2
    return trips, nfull - i


def block_state(nfull, tail, C):
    """(nfull class, tail class) of a block that has work."""
    return min(nfull, 9), ("none" if tail == 0 else "short" if tail < C // 4 else "long")


def trips_state(nfull):
    trips, left = ring(nfull)
    return (0,) if trips == 0 else (min(trips, 2), left)


def plain_call(n, d, row0, es, num_cus):
    """Everything the GPU test records and asserts about one pbn_debug_table_gram call: rec and the set of states its blocks reach."""
    C, nct = chunk_rows(es), nct_of(d)
    nblocks, _ = plain_blocks(n, num_cus)
    grid = plain_grid(nblocks, num_cus)
    states = {("grid", es, "capped" if grid < nblocks else "uncapped"), ("levels", es, reduce_levels(grid)), ("start", "plain", es, row0 % 4),
              ("start128", "plain", es, "on" if (row0 * es) % 128 == 0 else "off")}
    seen = set()
    for b in range(grid):
        _, _, mine, _, nfull, tail = plain_block(b, grid, n, C)
        if mine == 0 or (nfull, tail) in seen:
            continue
        seen.add((nfull, tail))
        states.add(("ring", "plain", es, nct) + block_state(nfull, tail, C))
        states.add(("trips", "plain", es) + trips_state(nfull))
        if tail:   # which block of the grid the cut chunk lands on
            states.add(("cut", es, "first" if b == 0 else "last" if b == grid - 1 else "middle"))
    return {"rec": [nblocks, grid, es, nct], "states": states}


# ---- segmented form ---------------------------------------------------------------------------------------------------------------------
def pieces(r0, r1):
    """scoring.hip compute_stats_segments: for (r = r0; r < r1; r += SEG_ROWS) piece [r, min(r + SEG_ROWS, r1))."""
    return [(r, min(r + SEG_ROWS, r1)) for r in range(r0, r1, SEG_ROWS)]


def seg_runs(count):
    """gram_seg_reduce_kernel: len = (count + 3) / 4; run q adds slots [q len, min(count, (q + 1) len)) in slot order, then
    ((run0 + run1) + run2) + run3."""
    ln = ceil_div(count, 4)
    return [(min(count, q * ln), min(count, (q + 1) * ln)) for q in range(4)]


def pair_launches(n):
    """Column sets of compute_stats_segments' launches: all n columns up to 64, else every pair bi < bj of 32-column blocks."""
    if n <= 64:
        return [list(range(n))]
    nb = ceil_div(n, PAIR_BLOCK)
    blk = [list(range(b * PAIR_BLOCK, min(n, b * PAIR_BLOCK + PAIR_BLOCK))) for b in range(nb)]
    return [blk[i] + blk[j] for i in range(nb) for j in range(i + 1, nb)]


def sse_pairs(d):
    """Column POSITION sets of pbn_table_sse's launches above 64 columns: every pair I <= J of 32-column blocks, I u J."""
    nb = ceil_div(d, PAIR_BLOCK)
    blk = [list(range(b * PAIR_BLOCK, min(d, b * PAIR_BLOCK + PAIR_BLOCK))) for b in range(nb)]
    return [(i, j, blk[i] + (blk[j] if j != i else [])) for i in range(nb) for j in range(i, nb)]


def super_blocks(length):
    """scoring.hip add_region: b_i = i == SB ? len : min(len, ceil64(len i / SB)); segment i = [max so far, max(prev, b_i))."""
    out, prev = [], 0
    for i in range(1, SUPER_BLOCKS + 1):
        b = length if i == SUPER_BLOCKS else (length * i // SUPER_BLOCKS + 63) // 64 * 64
        b = min(b, length)
        out.append((prev, max(prev, b)))
        prev = max(prev, b)
    return out


def segment_call(segs, n, es):
    """One pbn_debug_scoredata_segments call on the ranges segs = [(r0, r1)] of a table of n columns."""
    C = chunk_rows(es)
    launches = pair_launches(n)
    ncts = sorted({nct_of(len(c)) for c in launches})
    npieces = 0
    states = {("launches", es, len(launches))}
    seen = set()
    for r0, r1 in segs:
        ps = pieces(r0, r1)
        npieces += len(ps)
        states.add(("pieces", es, len(ps)))
        if r1 > r0:
            states.add(("start", "segmented", es, r0 % 4))
            states.add(("start128", "segmented", es, "on" if (r0 * es) % 128 == 0 else "off"))
        for first, end in ps:
            _, _, _, _, nfull, tail = piece_block(first, end, C)
            if (nfull, tail) in seen:
                continue
            seen.add((nfull, tail))
            for nct in ncts:
                states.add(("ring", "segmented", es, nct) + block_state(nfull, tail, C))
            states.add(("trips", "segmented", es) + trips_state(nfull))
    return {"rec": [npieces, len(launches) if npieces else 0, es, nct_of(len(launches[-1])) if npieces else 0], "states": states}


# ---- the planned cases (tests/test_gram_shapes_gpu.py) ------------------------------------------------------------------------------------
D_ALL = (1, 15, 16, 17, 31, 33, 47, 49, 64)          # NCT 1 .. 4 with last tiles of 1, 15 and 16 live columns
D_WIDE = (65, 70, 97, 130)                           # pbn_table_sse's 32-column block pairs
N_UNCAPPED = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4095, 4097, 16 * 256 + 1,
              191)                                   # one block of a double table with two whole chunks and a cut one of more than a wave's share
ROW0_UNCAPPED = (0, 1, 2, 3, 37)                     # mod 4: the 16-byte DMA's alignment on float tables, mod 2 on double ones; 37: off the line
D_CAPPED = (1, 49,                                   # NCT 1 and 4 with ONE live column in the last tile: the columns a stage's last DMA
            16, 48)                                  # instruction moves are dead there - so also NCT 1 and 3 with every column live
K_CAPPED = (4, 5, 6, 7, 8)
ROW0_CAPPED = (0, 3)
SEG_WIDTHS = (1, 17, 33, 49, 64, 65, 70, 97)
SEG_TAILS = (1, 2, 3, 4, 5, 8, 9, 10, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 63)
SEG_TAILS_F32 = (64, 65, 95, 96, 97, 127)
SEG_PIECES = (1, 2, 3, 4, 5, 8)
SEG_STARTS = (0, 1, 2, 3, 37)                        # added to a multiple of 64: 0 .. 3 mod 4 and one off the 128-byte line
SEG_TABLE_ROWS = 40001
PILOT_N = (1, 255, 1023, 1024, 1025, 5000)
NCOL_PLAIN = 64                                      # columns of the uncapped tables
NCOL_CAPPED = 49


def uncapped_cases():
    return [(n, row0) for n in sorted(set(N_UNCAPPED)) for row0 in ROW0_UNCAPPED]


def uncapped_table_rows():
    return max(N_UNCAPPED) + max(ROW0_UNCAPPED)


def capped_cases(num_cus, es, k):
    """(n, row0) with n = k B C + r, B = 2 num_cus blocks, C rows per chunk, r in (0, 1, C - 1, C, B C / 2 + 17): whole chunks only, or a cut
    chunk on the grid's first block or on a middle one; and r = -1, which puts it on the last block."""
    B, C = GD_BLOCKS_PER_CU * num_cus, chunk_rows(es)
    return [(k * B * C + r, row0) for r in (-1, 0, 1, C - 1, C, B * C // 2 + 17) for row0 in ROW0_CAPPED]


def capped_table_rows(num_cus, es):
    return max(n + row0 for k in K_CAPPED for n, row0 in capped_cases(num_cus, es, k))


def segment_lengths(es):
    C = chunk_rows(es)
    L = [0]
    L += [k * C + t for k in range(10) for t in (0, 1, C - 1)]   # k = 9: the class "nfull >= 9" with a cut chunk behind it
    tails = SEG_TAILS + (SEG_TAILS_F32 if es == 4 else ())
    L += [k * C + t for k in (0, 1, 5) for t in tails]
    L += [m * SEG_ROWS + t for m in SEG_PIECES for t in (0, 1, 77)]
    return sorted(set(L))


def multi_piece_lengths():
    return sorted(m * SEG_ROWS + t for m in SEG_PIECES for t in (0, 1, 77) if m * SEG_ROWS + t > SEG_ROWS)


def segment_cases(es, lengths=None, rows=SEG_TABLE_ROWS):
    """[(r0, r1)]: every length at the five starts; the bases walk through the table in steps of 64 rows so that the ranges overlap and
    stay inside it."""
    out = []
    for i, ln in enumerate(segment_lengths(es) if lengths is None else lengths):
        room = (rows - max(SEG_STARTS) - ln) // 64
        assert room >= 1
        for j, a in enumerate(SEG_STARTS):
            base = 64 * ((37 * i + 11 * j) % room)
            out.append((base + a, base + a + ln))
    return out


def required_states(num_cus):
    """What test_every_ring_state_was_seen asks for.  Segmented form: every NCT x nfull class x tail class of a piece (a piece without whole
    chunks has a cut one).  Plain form: below the cap rpb <= 256 rows, so a block owns at most M = 256 / C chunks (4 double, 2 float) - M
    whole ones, or up to M - 1 and a cut one - and the cases there run all d.  More chunks per block need the capped grid, whose cases run
    d = 1, 16, 48 and 49 (NCT 1, 3 and 4) at k = 4 .. 8 chunks per block: nfull 4 .. 8 with and without a cut chunk, and nfull 9 on the blocks in front
    of the one that holds the cut chunk.  A third level of the reduce tree needs more than 256 partials, that is more than 128 CUs."""
    req = set()
    for es in (8, 4):
        for nct in (1, 2, 3, 4):
            for nf in NFULL_CLASSES:
                for tail in TAILS:
                    if (nf, tail) != (0, "none"):
                        req.add(("ring", "segmented", es, nct, nf, tail))
            M = 256 // chunk_rows(es)
            req |= {("ring", "plain", es, nct, nf, "none") for nf in range(1, M + 1)}
            req |= {("ring", "plain", es, nct, nf, tail) for nf in range(M) for tail in ("short", "long")}
        for nct in sorted({nct_of(d) for d in D_CAPPED}):
            req |= {("ring", "plain", es, nct, nf, tail) for nf in (4, 5, 6, 7, 8) for tail in TAILS}
            req.add(("ring", "plain", es, nct, 9, "none"))
        for form in ("plain", "segmented"):
            req |= {("trips", form, es, 0), ("trips", form, es, 1, 3), ("trips", form, es, 1, 4), ("trips", form, es, 2, 3), ("trips", form, es, 2, 4)}
            req |= {("start", form, es, a) for a in range(4)}
            req |= {("start128", form, es, "on"), ("start128", form, es, "off")}
        req |= {("grid", es, "capped"), ("grid", es, "uncapped")}
        req |= {("levels", es, lv) for lv in (1, 2, 3) if lv < 3 or GD_BLOCKS_PER_CU * num_cus > REDUCE_ARITY ** 2}
        req |= {("cut", es, where) for where in ("first", "middle", "last")}
        req |= {("pieces", es, p) for p in (0, 1, 2, 3, 4, 5, 9)}
        req |= {("launches", es, 1), ("launches", es, 3), ("launches", es, 6)}
    return req


def planned_states(num_cus):
    """The states of every exact-leg call of the GPU test on a device of num_cus CUs."""
    got = set()
    for es in (8, 4):
        for d in D_ALL:
            for n, row0 in uncapped_cases():
                got |= plain_call(n, d, row0, es, num_cus)["states"]
        for d in D_CAPPED:
            for k in K_CAPPED:
                for n, row0 in capped_cases(num_cus, es, k):
                    got |= plain_call(n, d, row0, es, num_cus)["states"]
        for n in SEG_WIDTHS:
            got |= segment_call(segment_cases(es), n, es)["states"]
    return got


# ---- references -------------------------------------------------------------------------------------------------------------------------
class BlockGram:
    """Sums and products of the columns of X over any row range, from per-block sums (BLOCK rows each) added block by block plus the two
    edges: no difference of prefixes, so nothing cancels.  acc = np.float64 for integer-valued X (every partial sum is an integer below
    2^53: exact whatever the order, asserted by exact_headroom) or np.longdouble for the rounding leg."""
    BLOCK = 1024

    def __init__(self, X, acc):
        self.X = np.ascontiguousarray(X, dtype=acc)
        n = len(self.X)
        self.nb = n // self.BLOCK
        self.S = np.array([self._s(b * self.BLOCK, (b + 1) * self.BLOCK) for b in range(self.nb)]).reshape(self.nb, self.X.shape[1])
        self.G = np.array([self._g(b * self.BLOCK, (b + 1) * self.BLOCK) for b in range(self.nb)]).reshape(self.nb, self.X.shape[1], self.X.shape[1])

    def _s(self, a, b):
        return self.X[a:b].sum(axis=0)

    def _g(self, a, b):
        x = self.X[a:b]
        return x.T @ x if x.dtype == np.float64 else np.einsum("ri,rj->ij", x, x)   # (numpy's longdouble matmul is the slower of the two)

    def range(self, r0, r1):
        """(S [c], G [c][c]) over rows [r0, r1)."""
        b0, b1 = ceil_div(r0, self.BLOCK), r1 // self.BLOCK
        if b1 <= b0:
            return self._s(r0, r1), self._g(r0, r1)
        S = self._s(r0, b0 * self.BLOCK) + self.S[b0:b1].sum(axis=0) + self._s(b1 * self.BLOCK, r1)
        G = self._g(r0, b0 * self.BLOCK) + self.G[b0:b1].sum(axis=0) + self._g(b1 * self.BLOCK, r1)
        return S, G


def exact_headroom(rows, amp=15):
    """The largest |sum| the exact leg can form over `rows` rows of integers in [-amp, amp]: must stay below 2^53."""
    return rows * amp * amp
