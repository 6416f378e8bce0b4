"""Inputs that drive equal, opposite and empty operands through every point addition behind k_accumulate: the span
fix-up, the row / column sums, the bit planes, the per-window Horner, the final Horner, the segment path below c = 10 and
k_sum_points.  Plain Python, no device; tests/test_tail_cases_cpu.py proves that the inputs are what they claim and
tests/test_gpu_tail_cases.py runs them on the engine.

Two ideas carry everything here.

Expected values from discrete logs.  Every base is a known multiple m_i G of the generator and lives on the host as the
integer m_i mod r, so the expected MSM result is (sum_i k_i m_i mod r) G: one scalar multiplication of the oracle (or of
tests/mnt_model.py) whatever n is, and every intermediate sum of the pipeline has a discrete log that plain integer
arithmetic can follow.

Scalars composed from digits.  With window_bits = c forced and the endomorphism split off, the signed recoding of libff
(field_get_signed_digit) is the unique balanced representation k = sum_w s_w 2^(cw), -2^(c-1) <= s_w < 2^(c-1): a scalar
composed from such digits recodes to exactly those digits, and entry i lands in bucket |s_w| - 1 of window w with the sign
of s_w.  The bucket of weight 2^(c-1) is only reachable as s_w = -2^(c-1), which is what the raw digit 2^(c-1) recodes to
with a carry of +1 into the next window.  Constructions fill the windows 0 .. full_windows(c) - 1, chosen so that every
digit pattern stays below r (the top window only holds digits below r >> c(W-1)).

Every builder documents which adder it aims at and why the case fires WHATEVER the order of summation is: the guarantees
are statements about the multiset of bucket values (all equal; any two differ in sign in some input of the family), not
about q_row, RED_FOLD, the lane length or any other constant of today's schedule, so that a rewrite of the tail keeps
these tests meaningful.  Two builders are tied to a decomposition and say so: hp_cases (bit planes) and z_cases (the
row / column matrix).  If the tail stops using planes or the matrix, REPLACE those two with the collisions of whatever
intermediate sums the new tail has -- do not delete them.

Matrix of the device tests (tests/test_gpu_tail_cases.py): c in SEGMENT_CS below the row / column threshold, ROWCOL_CS
above it (even and odd column bits); c = 13 only for the 8- to 12-word prime-field G1 groups (WIDE groups -- Fq2 and the
24-word field -- stop at 12, their reductions run one wave per SIMD and the extra window size only costs time).
"""
import numpy as np

SEGMENT_CS = [4, 7, 9]
ROWCOL_CS = [10, 11, 12, 13]
P0 = 3   # discrete log of "the point P" of the uniform constructions


def signed_digits(k, c, W):
    """field_get_signed_digit (field_utils.tcc:167-203) for windows 0 .. W-1 of the plain integer k."""
    out, carry = [], 0
    for w in range(W):
        d = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        if d >> c:                      # overflow: digit 0, carry on
            out.append(0)
            carry = 1
        elif (d >> (c - 1)) & 1:
            out.append(d - (1 << c))
            carry = 1
        else:
            out.append(d)
            carry = 0
    return out


class Case:
    """palette: discrete logs of the distinct bases; base_idx[i] indexes it; digits[i, w]: planned signed digit of scalar i.
    meta: what the CPU file checks beyond digits and value (see each builder)."""

    def __init__(self, name, c, W, palette, base_idx, digits, doc, **meta):
        self.name, self.c, self.W, self.doc, self.meta = name, c, W, doc, meta
        self.palette = [int(m) for m in palette]
        self.base_idx = np.asarray(base_idx, dtype=np.int64)
        self.digits = np.asarray(digits, dtype=np.int64).reshape(len(self.base_idx), W)
        self._scalars = None

    @property
    def n(self):
        return len(self.base_idx)

    def scalars(self):
        """plain integer scalars sum_w s_w 2^(cw)"""
        if self._scalars is None:
            cache = {}
            out = []
            for row in self.digits.tolist():
                key = tuple(row)
                k = cache.get(key)
                if k is None:
                    k = cache[key] = sum(s << (self.c * w) for w, s in enumerate(row) if s)
                out.append(k)
            self._scalars = out
        return self._scalars

    def dlogs(self):
        return [self.palette[j] for j in self.base_idx.tolist()]

    def expected(self, r):
        return sum(k * m for k, m in zip(self.scalars(), self.dlogs())) % r

    def bucket_values(self, r):
        """{(window, weight): discrete log of the bucket's sum} over the non-empty buckets"""
        out = {}
        for row, m in zip(self.digits.tolist(), self.dlogs()):
            for w, s in enumerate(row):
                if s:
                    key = (w, abs(s))
                    out[key] = (out.get(key, 0) + (m if s > 0 else -m)) % r
        return out

    def window_sums(self, r):
        out = [0] * self.W
        for (w, wt), v in self.bucket_values(r).items():
            out[w] = (out[w] + wt * v) % r
        return out

    def padded(self, n):
        """the same MSM with zero scalars appended (batches want one length)"""
        extra = n - self.n
        assert extra >= 0
        return Case(self.name, self.c, self.W, self.palette, np.concatenate([self.base_idx, np.zeros(extra, dtype=np.int64)]),
                    np.concatenate([self.digits, np.zeros((extra, self.W), dtype=np.int64)]), self.doc, **self.meta)


# ------------------------------------------------------------------ group families
def _limbs(vals, fl):
    buf = b"".join(int(v).to_bytes(fl * 8, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).reshape(len(vals), fl).copy()


class PortFamily:
    """one of common.GROUPS through the C oracle (oracle/port.py)"""

    def __init__(self, port, name, curve, group):
        from common import golden, to_int
        self.port, self.name, self.curve, self.group = port, name, curve, group
        self.r = to_int(golden()[f"{name.rsplit('_g', 1)[0]}_g1/fr_modulus"])
        s = port.sizes(curve, group)
        self.fr_bits, self.fl = s["fr_bits"], s["fr_bytes"] // 8
        self.one, self.zero = port.group_consts(curve, group)
        self._pts, self._exp = {}, {}

    def scalars_mont(self, ks):
        if not len(ks):
            return np.zeros((0, self.fl), dtype=np.uint64)
        return self.port.fr_from_bigint(self.curve, _limbs([k % self.r for k in ks], self.fl))

    def point(self, m):
        """special-form record of m G, m any integer"""
        m %= self.r
        if m not in self._pts:
            p, neg = self.port, m > self.r // 2
            a = self.r - m if neg else m
            if a == 0:
                rec = self.zero.copy()
            elif a < (1 << 63):
                rec = p.bases_seq(self.curve, self.group, 1, first=a - 1)[0]
            else:
                rec = p.group_op(self.curve, self.group, 4, p.scalar_mul(self.curve, self.group, self.one, self.scalars_mont([a])[0]))
            self._pts[m] = p.group_op(self.curve, self.group, 3, rec) if neg and a else rec
        return self._pts[m]

    def bases(self, case):
        return np.stack([self.point(m) for m in case.palette])[case.base_idx]

    def expected_record(self, dlog):
        """affine record of dlog G as the engine returns it with out_form = OUT_AFFINE"""
        dlog %= self.r
        if dlog not in self._exp:
            p = self.port
            self._exp[dlog] = p.group_op(self.curve, self.group, 4,
                                         p.scalar_mul(self.curve, self.group, self.one, self.scalars_mont([dlog])[0]))
        return self._exp[dlog]

    def same(self, got, dlog):
        return bool((np.asarray(got) == self.expected_record(dlog)).all())

    def msm(self, bases, scalars_mont):
        p = self.port
        return p.multi_exp(self.curve, self.group, bases, scalars_mont, p.BDLO12_SIGNED, p.FORM_SPECIAL)


class MntFamily:
    """MNT4-298 G1 / G2 and MNT6-298 G1 through the pure-integer model (tests/mnt_model.py)"""

    def __init__(self, name, curve, group, model):
        self.name, self.curve, self.group, self.model = name, curve, group, model
        self.r, self.fr_bits = model.r, model.r.bit_length()
        self._pts, self._exp = {}, {}

    def scalars_mont(self, ks):
        return self.model.scalars_mont(ks)

    def _affine(self, m):
        m %= self.r
        if m not in self._exp:
            neg = m > self.r // 2
            P = self.model.mul(self.r - m if neg else m, self.model.one)
            self._exp[m] = self.model.neg(P) if neg else P
        return self._exp[m]

    def point(self, m):
        m %= self.r
        if m not in self._pts:
            self._pts[m] = self.model.records([self._affine(m)])[0]
        return self._pts[m]

    def bases(self, case):
        return np.stack([self.point(m) for m in case.palette])[case.base_idx]

    def same(self, got, dlog):
        return self.model.point(got) == self._affine(dlog)

    def msm(self, bases, scalars_mont):
        raise NotImplementedError("the model sums affine points: see test_tail_cases_cpu.py")


def num_windows(fam, c):
    """windows of the engine without the endomorphism split (field_get_signed_digit needs bits + 2)"""
    return (fam.fr_bits + 2 + c - 1) // c


def full_windows(fam, c):
    """Windows 0 .. Wu-1 take every digit -2^(c-1) .. 2^(c-1)-1 with the value (and a carry into window Wu) below r."""
    W = num_windows(fam, c)
    Wu = W - 1
    while Wu > 1 and (1 << (c - 1)) * sum(1 << (c * w) for w in range(Wu)) + (1 << (c * Wu)) >= fam.r:
        Wu -= 1
    return Wu


def materialize(fam, case):
    """(bases, scalars_mont, dlog_expected, description) of a case for the family's group"""
    ks = case.scalars()
    assert all(0 <= k < fam.r for k in ks), case.name
    return fam.bases(case), fam.scalars_mont(ks), case.expected(fam.r), f"{case.name}: {case.doc}"


def _rows(W, spec):
    """digit rows from [(digit, windows)]"""
    out = np.zeros((len(spec), W), dtype=np.int64)
    for i, (d, ws) in enumerate(spec):
        for w in ws:
            out[i, w] = d
    return out


# ------------------------------------------------------------------ U: uniform buckets
def u_case(fam, c, top=False, copies=1):
    """U -- every bucket of weight 1 .. 2^(c-1)-1 (top=True: and 2^(c-1)) of windows 0 .. Wu-1 holds `copies` entries of the
    one point P, so every bucket sum is the same point copies * P.

    Aims at: the equal-operand (doubling) branch of every adder of the reduction -- rec_sum_add / rec_sum_fold of the row and
    column sums, jac_add of wave_group_sum[_r], sum_wide_add / jac_add_wide of the wide planes, xyzz_add of the segment path,
    and the final Horner.
    Fires whatever the order: the first addition of two finite operands anywhere in a window's reduction -- in any tree, serial
    run or butterfly -- adds two single buckets, which are equal; in a power-of-two butterfly over full groups every level
    does.  Sums of equally many buckets are equal again, so equal-length row sums, equal-length column sums and the first
    finite addition inside every bit plane double too.  All window sums are equal: the final Horner meets 2^c S + S.
    top=True: the scalar of the extra entry has the digit -2^(c-1) in every window and +1 in window Wu; its base is -P, so
    the top bucket holds +P and window Wu holds the lone -P."""
    W, Wu, B = num_windows(fam, c), full_windows(fam, c), 1 << (c - 1)
    spec = [(d, range(Wu)) for d in range(1, B) for _ in range(copies)]
    idx = [0] * len(spec)
    digits = _rows(W, spec)
    if top:
        extra = _rows(W, [(-B, range(Wu))] * copies)
        extra[:, Wu] = 1
        digits = np.concatenate([digits, extra])
        idx += [1] * copies
    return Case(f"U{'top' if top else ''}{'x%d' % copies if copies > 1 else ''}", c, W, [P0, -P0], idx, digits,
                "uniform buckets: every bucket sum equal", kind="U", windows=Wu, value=copies * P0, top=top)


# ------------------------------------------------------------------ A_j: sign patterns
def a_case(fam, c, j):
    """A_j -- as U, but the bucket of weight d holds -P where bit j of d is set.  One input per j = 0 .. c-2.

    Aims at: the opposite-operand branch (result infinity) and the infinity-operand branches of the same adders as U.
    Fires whatever the order: two distinct weights differ in some bit j, so WHICHEVER pair of buckets an implementation adds
    first is an opposite pair in at least one A_j and an equal pair in the others; sums collapse to infinity in the middle of
    the trees (pairs d, d ^ 2^j cancel) and infinity operands then meet finite ones at every later level.
    A window's sum is sum_d (-1)^bit_j(d) d P = -2^(j+c-2) P (the pairs d, d + 2^j contribute -2^j each)."""
    W, Wu, B = num_windows(fam, c), full_windows(fam, c), 1 << (c - 1)
    assert 0 <= j <= c - 2
    spec = [(d, range(Wu)) for d in range(1, B)]
    idx = [(d >> j) & 1 for d in range(1, B)]
    return Case(f"A{j}", c, W, [P0, -P0], idx, _rows(W, spec), f"sign pattern: -P where bit {j} of the weight is set",
                kind="A", windows=Wu, j=j, window_sum=-(1 << (j + c - 2)) * P0)


# ------------------------------------------------------------------ F: one bucket across many lanes
# populations: with 16 entries per accumulation lane (AMDMSM_ACC_S=16, which make_plan applies as given) 40 entries span 3
# lanes (closed in the lane's own thread), 320 span 20 (mid queue), 1040 span 65 (long queue), 12800 span 800 lanes (aligned
# 256-lane blocks folded first); at the planner's own lane length the same inputs land in whichever classes it chooses.
F_POPULATIONS = [40, 320, 1040, 12800]


def f_case(fam, c, n, kind):
    """F -- all n scalars equal, so every window has ONE bucket of n entries cut into lane partials by the accumulation.
    kind 'same': all bases P (every lane partial the same multiple of P -- partial + partial is a doubling, in the serial
    span sums and at every level of the fold); 'alt': P, -P alternating (partials are infinity or +-P: infinity operands and
    opposite pairs); 'halves': P for the first half, -P for the second (the partials cancel only in the fold, not inside a
    lane; the bucket ends at infinity).
    Aims at: rec_sum_add / rec_sum_fold of the fix-up on records of form (i).  Fires whatever the lane length: equal
    entries give equal partials for every cut into equal runs, and the last, shorter run is the one unequal operand."""
    W, Wu, B = num_windows(fam, c), full_windows(fam, c), 1 << (c - 1)
    row = [(1 + (5 * w + 2) % (B - 1)) if w < Wu else 0 for w in range(W)]
    idx = {"same": [0] * n, "alt": [i & 1 for i in range(n)], "halves": [int(i >= n // 2) for i in range(n)]}[kind]
    return Case(f"F{kind}{n}", c, W, [P0, -P0], idx, np.tile(np.array(row, dtype=np.int64), (n, 1)),
                f"one bucket of {n} entries per window ({kind})", kind="F", windows=Wu)


def f_forms_case(fam, c, t=None):
    """F forms -- every bucket value is t P, but the odd weights hold ONE entry t P (a record k_accumulate writes: form (i))
    and the even weights t copies of P spanning lanes (a record the fix-up writes: form (ii)).
    Aims at: the equal-points test of rec_sum_add between records of the two forms.  Fires whatever the order: it is a U
    input (all bucket sums equal), and both forms occur in every row, column and segment, so any first addition of two
    neighbouring weights mixes them."""
    W, Wu, B = num_windows(fam, c), full_windows(fam, c), 1 << (c - 1)
    t = t or (40 if c <= 11 else 24 if c == 12 else 12)   # n stays below 2^16, so the oracle's multi_exp checks every input
    spec, idx = [], []
    for d in range(1, B):
        if d & 1:
            spec.append((d, range(Wu)))
            idx.append(1)
        else:
            spec += [(d, range(Wu))] * t
            idx += [0] * t
    return Case(f"Fforms{t}", c, W, [P0, t * P0], idx, _rows(W, spec), "equal bucket values from single entries and from spans",
                kind="U", windows=Wu, value=t * P0, top=False)


# ------------------------------------------------------------------ H: collisions between windows
def h_case(fam, c, name, pattern, top=None):
    """H -- one entry per non-empty window, base m_w G with the one-digit scalar 2^(cw), so window w sums to m_w G.  The
    pattern is read from window `top` (default W-2) downwards: 'F' a fresh value, '=' the running value after its c doublings
    (the addition is a doubling), '-' its negative (the running value becomes infinity), '.' an empty window (after a '-': the
    skip-the-doublings branch of horner_chain; then 'F' refills).
    Aims at: jac_dbl_run28[q] + jac_add_wide / jac_add_seq of horner_chain, k_horner and k_horner_batch.  Fires by
    construction of the running discrete log, which no schedule changes: the Horner over window sums is the definition
    of the result."""
    W = num_windows(fam, c)
    top = W - 2 if top is None else top
    assert len(pattern) <= top + 1
    ops = pattern + "." * (top + 1 - len(pattern))
    run, palette, spec, steps = 0, [], [], []
    for i, op in enumerate(ops):
        w = top - i
        run = run * (1 << c) % fam.r
        if op == ".":
            add = 0
        elif op == "F":
            add = 5 + w
        else:
            assert run != 0, "= / - need a finite running value"
            add = run if op == "=" else -run % fam.r
        steps.append((w, op, run, add))
        if add:
            palette.append(add)
            spec.append((1, [w]))
        run = (run + add) % fam.r
    return Case(name, c, W, palette or [1], list(range(len(spec))), _rows(W, spec), f"Horner pattern {ops} from window {top}",
                kind="H", steps=steps, result=run)


def h_cases(fam, c):
    W = num_windows(fam, c)
    top = W - 2
    return [
        h_case(fam, c, "Hequal", "F" + "=" * top),
        h_case(fam, c, "Hskip", ("F=-..F-." * W)[:top + 1]),
        h_case(fam, c, "Hinf", "F" + "=" * (top - 1) + "-"),
        h_case(fam, c, "Htopempty", "F=F", top=2),
        h_case(fam, c, "Honlyw0", "F", top=0),
        h_case(fam, c, "Hinfthenw0", "F-" + "." * (top - 2) + "F"),
    ]


# ------------------------------------------------------------------ HP: collisions between planes
def hp_cases(fam, c):
    """HP -- TIED TO THE BIT-PLANE DECOMPOSITION (window sum = sum_k 2^k P_k, P_k = sum of the buckets whose weight has bit k,
    Horner over k with one doubling between planes and, for the groups of four planes k_window_horner gives a wave each, four
    doublings between groups).  In one window Q = G sits in the bucket of weight 2^(k+1) and +-2Q in the bucket of weight
    2^k: after the doubling the running value 2Q meets +-2Q.  The group step uses weights 2^(k+4) and +-16Q.  Window w takes
    k = w mod (number of k), so one MSM covers every k; the weight 2^(c-1) comes as the digit -2^(c-1) on the base -Q with
    its carry of -Q into the next window, which is left empty.  'sparse': the top plane alone, single planes, all planes empty.
    If the tail stops using planes, replace this builder by the collisions of its intermediate sums."""
    W, Wu = num_windows(fam, c), full_windows(fam, c)
    out = []
    for tag, dist, mult in (("in", 1, 2), ("grp", 4, 16)):
        if c - 1 - dist < 0:
            continue
        for sign, sname in ((1, "eq"), (-1, "neg")):
            ks = list(range(0, c - dist))          # weights 2^k and 2^(k+dist) <= 2^(c-1)
            part = 0
            while ks:
                spec, idx, w, plan = [], [], 0, []
                while ks and w + 2 <= Wu:
                    k = ks.pop(0)
                    hi = 1 << (k + dist)
                    if hi == 1 << (c - 1):
                        spec.append([(-hi, w), (1, w + 1)])
                        idx.append(1)
                    else:
                        spec.append([(hi, w)])
                        idx.append(0)
                    spec.append([(1 << k, w)])
                    idx.append(2)
                    plan.append((w, k, dist, sign * mult))
                    w += 2 if hi == 1 << (c - 1) else 1
                digits = np.zeros((len(spec), W), dtype=np.int64)
                for i, lst in enumerate(spec):
                    for d, ww in lst:
                        digits[i, ww] = d
                out.append(Case(f"HP{tag}{sname}{part}", c, W, [1, -1, sign * mult], idx, digits,
                                f"plane collisions, distance {dist}, {sname}", kind="HP", plan=plan))
                part += 1
    # sparse planes: top plane alone (window 0, carry into the empty window 1), single planes, an empty window, one low plane
    spec = [[(-(1 << (c - 1)), 0), (1, 1)]]
    idx = [1]
    w = 2
    for k in range(c - 1):
        if w + 2 > Wu:
            break
        spec.append([(1 << k, w)])
        idx.append(0)
        w += 2 if k % 3 == 0 else 1          # some empty windows in between
    digits = np.zeros((len(spec), W), dtype=np.int64)
    for i, lst in enumerate(spec):
        for d, ww in lst:
            digits[i, ww] = d
    out.append(Case("HPsparse", c, W, [1, -1], idx, digits, "single planes, the top plane alone, empty windows", kind="HPsparse"))
    return out


# ------------------------------------------------------------------ Z: sparse windows
def z_cases(fam, c):
    """Z -- TIED TO THE ROW / COLUMN MATRIX (weight = hi * C + lo, C = 2^(c // 2) columns, rows 0 .. R with row R holding the
    weight 2^(c-1) alone).  Windows with exactly one non-empty bucket at the extreme positions (weight 1, weight 2^(c-1), first
    and last column, first and last full row), exactly one non-empty row, exactly one non-empty column, and a fully empty window
    between two full ones: every other operand of every sum is infinity.  The segment path below c = 10 sees the same inputs as
    lone buckets at segment ends.  If the tail stops using the matrix, replace the positions, keep the idea."""
    W, Wu, B = num_windows(fam, c), full_windows(fam, c), 1 << (c - 1)
    h = c // 2
    C, R = 1 << h, B >> h
    windows = [("w", [1]), ("top", [B]), ("w", [C]), ("w", [C - 1]), ("w", [B - 1]), ("w", [max(1, (R - 1) * C)]),
               ("w", [x for x in range((R // 2) * C, (R // 2) * C + C) if 1 <= x < B]),
               ("w", [hi * C + C // 2 + 1 for hi in range(R) if hi * C + C // 2 + 1 < B]),
               ("w", list(range(1, B))), ("empty", []), ("w", list(range(1, B)))]
    out, part = [], 0
    while windows:
        spec, idx, w, layout = [], [], 0, []
        while windows and w + 2 <= Wu:
            kind, weights = windows.pop(0)
            layout.append((w, kind, weights))
            if kind == "top":
                spec.append([(-B, w), (1, w + 1)])
                idx.append(1)
                w += 2
                continue
            for d in weights:
                spec.append([(d, w)])
                idx.append(0)
            w += 1
        digits = np.zeros((len(spec), W), dtype=np.int64)
        for i, lst in enumerate(spec):
            for d, ww in lst:
                digits[i, ww] = d
        out.append(Case(f"Z{part}", c, W, [P0, -P0], idx, digits, "sparse windows: lone buckets, one row, one column, an empty window",
                        kind="Z", layout=layout))
        part += 1
    return out


# ------------------------------------------------------------------ the families the device file runs
def cases_for(fam, c, family):
    """the named family of cases at window size c: 'U', 'A', 'F', 'H', 'HP', 'Z'"""
    if family == "U":
        return [u_case(fam, c), u_case(fam, c, top=True)]
    if family == "A":
        return [a_case(fam, c, j) for j in range(c - 1)]
    if family == "F":
        return [f_case(fam, c, n, kind) for n in F_POPULATIONS for kind in ("same", "alt", "halves")] + [f_forms_case(fam, c)]
    if family == "H":
        return h_cases(fam, c)
    if family == "HP":
        return hp_cases(fam, c)
    if family == "Z":
        return z_cases(fam, c)
    raise KeyError(family)


FAMILIES = ["U", "A", "F", "H", "HP", "Z"]


def knob_cases(fam, c):
    """what every alternative tail path runs: U, A_0, A_(c-2), F and HP"""
    return ([u_case(fam, c), u_case(fam, c, top=True), a_case(fam, c, 0), a_case(fam, c, c - 2)] + cases_for(fam, c, "F")
            + hp_cases(fam, c))


# partial results for k_sum_points (engine.sum_points): discrete logs, None = infinity.  Neighbours are equal, opposite or
# infinite, and so are the halves and quarters of the lists: a serial sum, a pairwise tree and a butterfly all meet them.
SUM_POINT_LISTS = [
    [5, 5],
    [5, -5],
    [None, None],
    [5, 5, 10, 20, 40],                    # a serial sum doubles at every step
    [5, 5, 5, 5, 5, 5, 5, 5],              # a tree doubles at every level
    [5, -5, 7, -7, 9, -9, 11, -11],        # pairs cancel: infinity + infinity above
    [5, 7, -5, -7],                        # halves cancel
    [None, 5, None, 5, None, -10, None],   # infinity between equal and opposite neighbours
    [3, None, None, 3, 6, -12, 4, 4, 8],
    [9],
    [None],
]
