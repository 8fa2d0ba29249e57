"""A lane-by-lane model of bftkv_amd/csrc/mont28.h with Python's unbounded integers: `mont_mul` on the ring window and on
the window that normalises at block boundaries, its squaring form, the final cross-lane carry hop, `canonicalize` and
`reduce_once`.

It mirrors the header's structure, not only its value: every lane owns L limbs and its own column accumulators, the
columns sit where the header puts them (ring index (O + j) % 2L, or the re-aligned window), a lane takes from the next lane
what DPP row_shl:1 gives it (the low 32 bits of a column that lane has retired, masked to 28 bits; 0 past the end of a row of
16 lanes), the Montgomery factor is group lane 0's, and the carries hop lane to lane the way grp_shr1 moves them.  Where the
header truncates to 32 bits the model does; where it keeps 64 bits the model keeps ALL bits and records the largest value a
column held, which is how the header's claim that 64 bits suffice becomes a measured number (tests/test_mont_model.py).

It is an oracle (tests/test_gpu_mont_forms.py compares the device's limbs with it) and a tool: `Stats` says how far a carry
or a borrow travelled, which is what the operand search of tests/mont_cases.py maximises.  `mut` names deliberate defects,
used to show which cases notice them."""

W = 28
MASK = (1 << W) - 1
U32 = 0xFFFFFFFF
ROW = 16                                          # lanes of a DPP row
FORMS = {(19, 4): 2048, (10, 8): 2048, (14, 8): 3072, (19, 8): 4096}     # (L, TPI) -> largest modulus it is used for

MUT_NO_MASK = "no_mask"                           # the limb read from the next lane keeps all its 32 bits
MUT_ROW_END = "row_end_reads_neighbour"           # lane 15 of a row reads lane 0 of the next row instead of 0
MUT_CANON_HOP = "canon_one_hop_fewer"             # canonicalize runs TPI - 1 steps
MUT_CANON_2HOPS = "canon_two_hops_fewer"          # ... TPI - 2
BOUND_M = "m_forced_to_maximum"                   # no defect but a bound: every row's Montgomery factor taken as 2^28 - 1


def is_norm(L, TPI):
    return 2 * TPI * L > 255                      # the header's NORM


def to_limbs(x, N):
    assert 0 <= x < 1 << (W * N)
    return [(x >> (W * i)) & MASK for i in range(N)]


def from_limbs(row):
    return sum(int(v) << (W * i) for i, v in enumerate(row))


def n0inv_of(n):
    return (-pow(n, -1, 1 << W)) & MASK


class Stats:
    """What a run saw: the largest column accumulator, the largest output limb of mont_mul, how often the cross-lane hop's
    ripple reached the third limb, and the longest run of consecutive lane-to-lane steps in which a carry (canonicalize) or a
    borrow (reduce_once) moved on."""

    def __init__(self):
        self.max_col = 0
        self.max_limb = 0
        self.hop_third = 0
        self.canon_hops = 0
        self.borrow_hops = 0

    def col(self, v):
        if v > self.max_col:
            self.max_col = v


def _shl1(vals, i, mut):
    """DPP row_shl:1 with bound_ctrl: lane i takes lane i + 1's value inside its row of 16, 0 past the end."""
    if i + 1 >= len(vals):
        return 0
    if i % ROW == ROW - 1 and MUT_ROW_END not in mut:
        return 0
    return vals[i + 1]


def _incoming(Q, idx, mut):
    nl = len(Q)
    lo = [Q[i][idx] & U32 for i in range(nl)]
    keep = U32 if MUT_NO_MASK in mut else MASK
    return [_shl1(lo, i, mut) & keep for i in range(nl)]


def _rows(Q, cols, ap, b, n, n0inv, L, TPI, sqr, stats, mut, ring):
    """The L rows of one block.  cols(r, k) is where window column r + k lives.  The MAC that opens a fresh column (k = L - 1,
    r > 0) takes as its addend, on the ring, the limb the next lane retired one row earlier; on the normalising window 0, or
    in row 1 the seed the last normalisation left in column L."""
    nl = len(Q)
    for r in range(L):
        inc = _incoming(Q, cols(r - 1, 0), mut) if (r > 0 and ring) else None
        k0 = r if sqr else 0
        idx = [cols(r, k) for k in range(L)]
        last = idx[L - 1]
        for i in range(nl):
            ai = ap[i // TPI][r] & U32
            ai2 = (ai << 1) & U32                 # SQR: off-diagonal products count twice
            q, bi = Q[i], b[i]
            if r > 0:                             # first touch of the fresh column: assigned, not accumulated
                q[last] = inc[i] if ring else q[last] if r == 1 else 0
            if sqr:
                q[idx[r]] += ai * bi[r]
                for j, bk in zip(idx[r + 1:], bi[r + 1:]):
                    q[j] += ai2 * bk
            else:
                for j, bk in zip(idx, bi):
                    q[j] += ai * bk
        for g in range(nl // TPI):
            m = MASK if BOUND_M in mut else (((Q[g * TPI][idx[0]] & U32) * n0inv[g]) & U32) & MASK
            for i in range(g * TPI, g * TPI + TPI):
                q = Q[i]
                for j, nk in zip(idx, n[i]):
                    q[j] += m * nk
        for i in range(nl):
            q = Q[i]
            if stats is not None:
                stats.col(max(q))
            q[cols(r + 1, 0)] += q[idx[0]] >> W
            if stats is not None:
                stats.col(q[cols(r + 1, 0)])


def mont_mul_lanes(groups, L, TPI, sqr=False, stats=None, mut=()):
    """mont_mul<L, TPI, sqr> of adjacent groups of one wave, lane by lane.  groups: (a, b, n, n0inv) with limb rows of
    N = L * TPI entries (b is ignored when sqr: the header is given the same number twice).  Returns the lazy output rows."""
    N = L * TPI
    ng = len(groups)
    nl = ng * TPI
    ap_all = [list(g[0]) for g in groups]
    b = [list((g[0] if sqr else g[1])[(i % TPI) * L:(i % TPI) * L + L]) for g in groups for i in range(TPI)]
    n = [list(g[2][(i % TPI) * L:(i % TPI) * L + L]) for g in groups for i in range(TPI)]
    n0inv = [g[3] for g in groups]
    for g in groups:
        assert len(g[0]) == N and len(g[2]) == N and (sqr or len(g[1]) == N)
    norm = is_norm(L, TPI)
    M = 2 * L
    Q = [[0] * (2 * L - 1 if norm else M) for _ in range(nl)]

    if not norm:
        for blk in range(TPI):
            O = (blk % 2) * L
            ap = [a[blk * L:blk * L + L] for a in ap_all]
            _rows(Q, lambda r, k, O=O: (O + r + k) % M, ap, b, n, n0inv, L, TPI, sqr, stats, mut, True)
            # the limb retired by the block's last row: column L - 1 of the next block, or the result's top limb
            inc = _incoming(Q, (O + L - 1) % M, mut)
            for i in range(nl):
                Q[i][(O + M - 1) % M] = inc[i]
    else:
        for blk in range(TPI):
            ap = [a[blk * L:blk * L + L] for a in ap_all]
            _rows(Q, lambda r, k: r + k, ap, b, n, n0inv, L, TPI, sqr, stats, mut, False)
            # re-align: new Q[k] = own Q[L + k] + the next lane's retired column k
            for k in range(L):
                inc = _incoming(Q, k, mut)
                for i in range(nl):
                    Q[i][k] = Q[i][L + k] + inc[i] if k < L - 1 else inc[i]
            for i in range(nl):
                q = Q[i]
                if stats is not None:
                    stats.col(max(q[:L]))
                for k in range(L):
                    c = q[k] >> W
                    q[k] &= MASK
                    if k < L - 1:
                        q[k + 1] += c
                        if stats is not None:
                            stats.col(q[k + 1])
                    else:
                        q[L] = c

    # lazy normalisation: local ripple, one cross-lane hop, a ripple over two limbs
    out = [[0] * L for _ in range(nl)]
    cs = []
    for i in range(nl):
        c = 0
        for k in range(L):
            v = Q[i][k] + c
            if stats is not None:
                stats.col(v)
            out[i][k] = v & MASK
            c = v >> W
        if norm:
            c += Q[i][L]
        if stats is not None:
            stats.col(c)
        cs.append(c)
    for i in range(nl):
        # two 32-bit halves of the carry go through grp_shr1: what a 64-bit register holds of it
        cin = 0 if i % TPI == 0 else cs[i - 1] & 0xFFFFFFFFFFFFFFFF
        v0 = out[i][0] + cin
        out[i][0] = v0 & MASK
        v1 = (out[i][1] + ((v0 >> W) & U32)) & U32
        out[i][1] = v1 & MASK
        out[i][2] = (out[i][2] + (v1 >> W)) & U32
        if stats is not None and v1 >> W:
            stats.hop_third += 1
    rows = [sum((out[g * TPI + l] for l in range(TPI)), []) for g in range(ng)]
    if stats is not None:
        stats.max_limb = max(stats.max_limb, max(max(r) for r in rows))
    return rows


def mont_mul(a, b, n, n0inv, L, TPI, sqr=False, stats=None, mut=()):
    """One group alone in its row."""
    return mont_mul_lanes([(a, b, n, n0inv)], L, TPI, sqr, stats, mut)[0]


def _longest_run(moved):
    """moved[step][lane] is true when a non-zero carry entered `lane` in `step`: the longest chain lane -> lane + 1 -> ... over
    consecutive steps."""
    best = 0
    run = {}
    for flags in moved:
        new = {}
        for lane, f in enumerate(flags):
            if f:
                new[lane] = run.get(lane - 1, 0) + 1
                best = max(best, new[lane])
        run = new
    return best


def canonicalize(x, L, TPI, stats=None, mut=()):
    """Every limb below 2^28: TPI steps, in each of which a lane takes the carry the lane below it produced in the step
    before and ripples it through its own limbs."""
    x = list(x)
    steps = TPI - (1 if MUT_CANON_HOP in mut else 2 if MUT_CANON_2HOPS in mut else 0)
    cout = [0] * TPI
    moved = []
    for _ in range(steps):
        cin = [0] + cout[:-1]
        moved.append([c != 0 for c in cin])
        for l in range(TPI):
            c = cin[l]
            for k in range(l * L, l * L + L):
                v = (x[k] + c) & U32
                x[k] = v & MASK
                c = v >> W
            cout[l] = c
    if stats is not None:
        stats.canon_hops = max(stats.canon_hops, _longest_run(moved))
    return x


def reduce_once(y, n, L, TPI, stats=None):
    """y - n when y >= n, for canonical y < 2n.  Returns (row, candidate): `candidate` is the top lane's limb comparison, the
    condition under which a wave runs the subtraction at all; a wave that holds another group's candidate runs it for every
    group, so the row is the subtraction's verdict either way and the caller checks that a non-candidate is left alone."""
    ge = 1
    for k in range((TPI - 1) * L, TPI * L):
        ge = 1 if y[k] > n[k] else (0 if y[k] < n[k] else ge)
    d = [y[k] - n[k] for k in range(L * TPI)]
    cout = [0] * TPI
    top = 0
    moved = []
    for _ in range(TPI):
        cin = [0] + cout[:-1]
        moved.append([c != 0 for c in cin])
        for l in range(TPI):
            c = cin[l]
            for k in range(l * L, l * L + L):
                v = d[k] + c
                d[k] = v & MASK
                c = v >> W                        # -1 = borrow
            cout[l] = c
        top += cout[TPI - 1]
    if stats is not None:
        stats.borrow_hops = max(stats.borrow_hops, _longest_run(moved))
    return (d if top == 0 else list(y)), bool(ge)


MUL, SQR, CHAIN = 0, 1, 2


def run_op(op, k, a, b, n, n0inv, L, TPI, stats=None, mut=()):
    """What the driver's kernel computes for one group: (lazy, canonical, reduced) limb rows."""
    if op == MUL:
        y = mont_mul(a, b, n, n0inv, L, TPI, False, stats, mut)
    elif op == SQR:
        y = mont_mul(a, a, n, n0inv, L, TPI, True, stats, mut)
    else:
        y = list(a)
        for _ in range(k):
            y = mont_mul(y, y, n, n0inv, L, TPI, True, stats, mut)
        y = mont_mul(b, y, n, n0inv, L, TPI, False, stats, mut)       # b is the broadcast operand, as k_rsa_modexp's x is
    c = canonicalize(y, L, TPI, stats, mut)
    r, cand = reduce_once(c, n, L, TPI, stats)
    assert cand or r == c, "reduce_once changed a number its top-lane comparison had ruled out"
    return y, c, r
