"""CPU-side checks of qmg::SolveLedger (include/qmg/krylov.hpp), the per-system book-keeping that the five lock-step Krylov cores share:
which systems of a batch run, stop, re-anchor and report.  tests/host/krylov_ledger_host.cpp is compiled with g++ against the header alone
(QMG_KRYLOV_HOST_ONLY) and driven by scripts; every answer is held to the rules as `Rules` states them below, in plain Python and without the
header, and every scenario to what it must show whatever the implementation.  All numbers are powers of two, so each recurrence value is
exact and the step at which a system stops is known beforehand.  Batches: 6 slots under 0x3F and 0x3B, 16 slots under 0xA5A5; a slot
outside the mask carries |b|^2 = 7 that nothing may look at."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = [(6, 0x3F), (6, 0x3B), (16, 0xA5A5)]
EPS = 2.0 ** -20


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("krylov_ledger") / "krylov_ledger_host")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-o", out, os.path.join(ROOT, "tests", "host", "krylov_ledger_host.cpp")])
    return out


def bits(m):
    return [k for k in range(32) if (m >> k) & 1]


class Rules:
    """The rules of the lock-step cores, one statement each (the header comment of krylov.hpp says them in words).  Every method appends the
    command to the script and the answer the rules give to `want`."""

    def __init__(self, bsq, mask, max_iter, eps, eps_k=None):
        n = len(bsq)
        self.n, self.mask, self.max_iter = n, mask, max_iter
        self.eps = list(eps_k) if eps_k else [eps] * n
        self.bsq = [b if (mask >> k) & 1 else 0.0 for k, b in enumerate(bsq)]        # a slot outside the mask does not exist
        self.zero_b = sum(1 << k for k in bits(mask) if self.bsq[k] == 0.0)          # x = 0 solves A x = 0: done before anything runs
        self.run = mask & ~self.zero_b
        self.act = 0
        self.rsq, self.ref = list(self.bsq), list(self.bsq)
        self.its, self.ops = [0] * n, [0] * n
        self.conv = [bool((self.zero_b >> k) & 1) for k in range(n)]
        self.handed = []                                                             # every mask an apply was handed
        self.script = ["ledger %d %x %d %r %d %s" % (n, mask, max_iter, eps, 1 if eps_k else 0, " ".join(repr(v) for v in list(bsq) + list(eps_k or [])))]
        self.want = ["masks %x %x 0" % (self.zero_b, self.run)]

    def small(self, k, c=1.0):
        return math.sqrt(self.rsq[k]) < c * self.eps[k] * math.sqrt(self.bsq[k])

    def open(self, m, r0=None):
        """a solve (or a CG cycle) opens for the systems of m: converged at the guess or active, none active without iterations to spend"""
        self.script.append("open_b %x" % m if r0 is None else "open %x %s" % (m, " ".join(repr(v) for v in r0)))
        self.act = 0
        for k in bits(m):
            self.rsq[k] = self.ref[k] = self.bsq[k] if r0 is None else r0[k]
            self.conv[k] = self.small(k)
            if not self.conv[k] and self.max_iter > 0:
                self.act |= 1 << k
        self.want.append("act %x" % self.act)

    def count(self, m):
        self.script.append("count %x" % m)
        self.handed.append(m)
        for k in bits(m):
            self.ops[k] += 1

    def recur(self, k, delta, c):
        self.script.append("recur %d %r %r" % (k, delta, c))
        self.rsq[k] -= delta
        ask = not (self.rsq[k] > 1e-8 * self.ref[k]) or self.small(k, c)
        self.want.append("renorm %d" % ask)
        return ask

    def anchor(self, k, t):
        self.script.append("anchor %d %r" % (k, t))
        self.rsq[k] = self.ref[k] = t

    def breakdown(self, k):
        self.script.append("breakdown %d" % k)
        self.act &= ~(1 << k)

    def settle(self, k, step=False):
        self.script.append("%s %d" % ("step" if step else "settle", k))
        self.its[k] += 1 if step else 0
        if self.small(k):
            self.conv[k] = True
            self.act &= ~(1 << k)
        self.want.append("done %d" % self.conv[k])
        return self.conv[k]

    def cap(self):
        self.script.append("cap")
        self.act &= ~sum(1 << k for k in bits(self.act) if self.its[k] >= self.max_iter)
        self.want.append("act %x" % self.act)

    def rows(self):
        self.script.append("rows")
        self.want.append("act %x" % self.act)
        for k in range(self.n):
            rel = math.sqrt(self.rsq[k]) / math.sqrt(self.bsq[k]) if self.bsq[k] > 0 else 0.0
            self.want.append("row %d %d %d %r %d %r %r" % (k, self.conv[k], self.its[k], self.rsq[k], self.ops[k], rel, self.ref[k]))


def same(a, b):
    """the same answer: masks and flags as text, numbers by value (%.17g there, repr here)"""
    ta, tb = a.split(), b.split()
    if ta[0] != tb[0] or len(ta) != len(tb):
        return False
    numeric = ta[0] == "row"
    return all(x == y or (numeric and float(x) == float(y)) for x, y in zip(ta[1:], tb[1:]))


def check(exe, tmp_path, rules):
    """run the script; every answer is the rules'; returns the closing rows {k: (success, iter, resSq, ops, rel, rsq_ref)} of the ledger"""
    rules.rows()
    fin, fout = str(tmp_path / "script.txt"), str(tmp_path / "out.txt")
    with open(fin, "w") as f:
        f.write("\n".join(rules.script) + "\n")
    subprocess.check_call([exe, fin, fout], timeout=60)
    got = open(fout).read().splitlines()
    assert len(got) == len(rules.want), (len(got), len(rules.want))
    for i, (g, w) in enumerate(zip(got, rules.want)):
        assert same(g, w), (i, g, w)
    rows = {}
    for g in got[-rules.n:]:
        t = g.split()
        rows[int(t[1])] = (int(t[2]), int(t[3]), float(t[4]), int(t[5]), float(t[6]), float(t[7]))
    for m in rules.handed:                                # no apply reaches a system outside the mask or one with a zero right-hand side
        assert m & ~rules.run == 0, hex(m)
    for k in range(rules.n):
        if not (rules.mask >> k) & 1:                     # 9: a masked-out slot keeps inversion_info's defaults
            assert rows[k] == (0, 0, 0.0, 0, 0.0, 0.0), (k, rows[k])
    return rows


def batch(nrhs, mask, zero_slot=None):
    """|b_k|^2 = 4^(k+1) for the systems of the mask (so system k's |b| = 2^(k+1)), 0 for `zero_slot`, 7 outside the mask"""
    return [(0.0 if k == zero_slot else 4.0 ** (k + 1)) if (mask >> k) & 1 else 7.0 for k in range(nrhs)]


def iterate(r, halvings, c, max_steps=200, breakdown=None, restart_every=0):
    """The loop of bmr_core (c = 4) / bgcr_core (c = 1) as they ask the ledger: one counted apply for the active mask, per system a
    breakdown or the recurrence rsq -= delta (here rsq / 4^halvings[k] is what remains), a true norm where asked for (the recurrence's own
    value), the step end, GCR's restart with its counted true residual, then the cap.  Returns the step at which each bit left."""
    left, gone, step = {}, 0, 0
    while r.act and step < max_steps:
        assert r.act & gone == 0                          # a bit that left never returns
        start = r.act
        r.count(r.act)
        upd = []
        for k in bits(r.act):
            if breakdown and breakdown.get(k) == step:
                r.breakdown(k)
                continue
            upd.append(k)
            if r.recur(k, r.rsq[k] - r.rsq[k] / 4.0 ** halvings[k], c):
                r.anchor(k, r.rsq[k])
        for k in upd:
            r.settle(k, step=True)
        step += 1
        if restart_every and step % restart_every == 0 and r.act:
            r.count(r.act)
            for k in bits(r.act):
                r.anchor(k, r.rsq[k])
                r.settle(k)
        r.cap()
        for k in bits(start & ~r.act):
            left[k] = step
        gone |= start & ~r.act
    return left


@pytest.mark.parametrize("nrhs,mask", LAYOUTS)
@pytest.mark.parametrize("guess", [False, True])
def test_zero_rhs_and_converged_at_the_guess(exe, tmp_path, nrhs, mask, guess):
    """1, 2: a zero |b|^2 is success / iter 0 / resSq 0 / ops 0 and in no mask; a system whose opening residual is below eps |b| has the
    opening apply alone (none under zero_guess, where it needs eps > 1: its residual is b) and is never active"""
    act0 = bits(mask)
    zero, at_guess = act0[1], act0[2]
    eps_k = [EPS] * nrhs
    if not guess:
        eps_k[at_guess] = 2.0                             # |r0| = |b| < 2 |b|
    r = Rules(batch(nrhs, mask, zero), mask, 50, EPS, eps_k)
    assert r.zero_b == 1 << zero and r.run == mask & ~(1 << zero)
    if guess:
        r.count(r.run)
        r.open(r.run, [r.bsq[k] * (2.0 ** -44 if k == at_guess else 0.25) for k in range(nrhs)])   # |r0| = 2^-22 |b| < eps |b|
    else:
        r.open(r.run)
    assert r.act == r.run & ~(1 << at_guess)
    iterate(r, [3] * nrhs, 4.0)
    rows = check(exe, tmp_path, r)
    assert rows[zero][:5] == (1, 0, 0.0, 0, 0.0)
    assert rows[at_guess][:2] == (1, 0) and rows[at_guess][3] == (1 if guess else 0)
    assert all(not (m >> zero) & 1 for m in r.handed) and all(not (m >> at_guess) & 1 for m in r.handed[1 if guess else 0:])
    assert all(rows[k][0] == 1 and rows[k][1] > 0 for k in bits(r.run) if k != at_guess)


@pytest.mark.parametrize("nrhs,mask", LAYOUTS)
@pytest.mark.parametrize("guess", [False, True])
def test_max_iter_zero(exe, tmp_path, nrhs, mask, guess):
    """3: no system is active and ops is the opening residual alone"""
    r = Rules(batch(nrhs, mask, bits(mask)[1]), mask, 0, EPS)
    if guess:
        r.count(r.run)
        r.open(r.run, [b * 0.25 for b in r.bsq])
    else:
        r.open(r.run)
    assert r.act == 0
    r.cap()
    rows = check(exe, tmp_path, r)
    for k in bits(r.run):
        assert rows[k][:4] == (0, 0, r.bsq[k] * (0.25 if guess else 1.0), 1 if guess else 0)
    assert len(r.handed) == (1 if guess else 0)


@pytest.mark.parametrize("nrhs,mask", LAYOUTS)
@pytest.mark.parametrize("c", [4.0, 1.0])
def test_scripted_sequences_stop_where_the_script_says(exe, tmp_path, nrhs, mask, c):
    """4: rsq falls by 4^h per step, |r| by 2^h, so a system is below eps |b| = 2^-20 |b| first after floor(20 / h) + 1 steps: three different
    stopping iterations in one batch, each bit leaving at its own and not coming back"""
    h = [(1, 2, 3)[k % 3] for k in range(nrhs)]
    r = Rules(batch(nrhs, mask), mask, 100, EPS)
    r.open(r.run)
    left = iterate(r, h, c)
    rows = check(exe, tmp_path, r)
    for k in bits(mask):
        stop = 20 // h[k] + 1
        assert rows[k][:2] == (1, stop) and rows[k][3] == stop and left[k] == stop, (k, rows[k], left.get(k))
        assert rows[k][2] == r.bsq[k] / 4.0 ** (h[k] * stop)
    assert len({rows[k][1] for k in bits(mask)}) == 3


@pytest.mark.parametrize("nrhs,mask", LAYOUTS)
@pytest.mark.parametrize("restart", [0, 4])
def test_cap_and_gcr_restart_order(exe, tmp_path, nrhs, mask, restart):
    """5: max_iter = 8.  A system that needs 21 steps leaves at 8 without success; one that needs 7 converges at 7.  With a restart every 4
    steps (GCR: restart, then cap) the restart at step 8 is counted for the capped systems, which were still active when it ran, and not
    for the system that converged at step 8 itself"""
    act0 = bits(mask)
    h = [1] * nrhs
    eps_k = [EPS] * nrhs
    fast, at8 = act0[0], act0[1]
    h[fast], h[at8], eps_k[at8] = 3, 2, 2.0 ** -15.5      # |r| = 4^-k |b|: below 2^-15.5 |b| first at k = 8
    r = Rules(batch(nrhs, mask), mask, 8, EPS, eps_k)
    r.open(r.run)
    left = iterate(r, h, 1.0, restart_every=restart)
    rows = check(exe, tmp_path, r)
    n_restarts = 2 if restart else 0
    assert rows[fast][:2] == (1, 7) and rows[fast][3] == 7 + (1 if restart else 0)
    assert rows[at8][:2] == (1, 8) and rows[at8][3] == 8 + (1 if restart else 0)          # the restart at 4 only
    for k in act0[2:]:
        assert rows[k][:2] == (0, 8) and rows[k][3] == 8 + n_restarts and left[k] == 8, (k, rows[k])
        assert rows[k][2] == r.bsq[k] / 4.0 ** 8


@pytest.mark.parametrize("nrhs,mask", LAYOUTS)
def test_breakdown(exe, tmp_path, nrhs, mask):
    """6: a system that breaks down in its 4th step leaves without success, iter 3, having been counted the apply of that step; the rest go on"""
    broken = bits(mask)[2]
    r = Rules(batch(nrhs, mask), mask, 100, EPS)
    r.open(r.run)
    left = iterate(r, [2] * nrhs, 4.0, breakdown={broken: 3})
    rows = check(exe, tmp_path, r)
    assert rows[broken][:4] == (0, 3, r.bsq[broken] / 4.0 ** 6, 4) and left[broken] == 4
    assert all(rows[k][:2] == (1, 11) for k in bits(mask) if k != broken)
    assert all(not (m >> broken) & 1 for m in r.handed[4:])


@pytest.mark.parametrize("nrhs,mask", LAYOUTS)
def test_reanchoring(exe, tmp_path, nrhs, mask):
    """7: eps = 2^-40, rsq falls by 4 per step from rsq_ref = |b|^2.  1e-8 lies between 4^-13 and 4^-14: the recurrence asks for a true norm
    at step 14 and not before; anchored there (on a value a little off the recurrence's, as a true norm is), rsq_ref follows and the next
    request comes 14 steps later.  Near convergence: |r| < 4 eps |b| first at step 39 (c = 4), |r| < eps |b| first at step 41 (c = 1)."""
    for c, first_small in ((4.0, 39), (1.0, 41)):
        r = Rules(batch(nrhs, mask), mask, 100, 2.0 ** -40)
        r.open(r.run)
        k = bits(mask)[-1]
        asked = []
        for step in range(1, 42):
            if r.recur(k, r.rsq[k] * 0.75, c):
                asked.append(step)
                r.anchor(k, r.rsq[k] * (1.0 + 2.0 ** -30))
                assert r.ref[k] == r.rsq[k]
            if step < first_small:
                r.settle(k, step=True)
        assert asked[:2] == [14, 28] and [s for s in asked if s > 28] == list(range(first_small, 42)), (c, asked)
        rows = check(exe, tmp_path, r)
        assert rows[k][5] == rows[k][2] != r.bsq[k]


@pytest.mark.parametrize("nrhs,mask", LAYOUTS)
def test_eps_per_system(exe, tmp_path, nrhs, mask):
    """8: two systems with the same |b|, the same rsq script (|r| halves per step) and eps_k = 2^-10 / 2^-30 stop at steps 11 and 31; the
    call's scalar eps (0.5 here) is not looked at once eps_per_system is given"""
    a, b = bits(mask)[0], bits(mask)[-1]
    bsq = batch(nrhs, mask)
    bsq[b] = bsq[a]
    eps_k = [EPS] * nrhs
    eps_k[a], eps_k[b] = 2.0 ** -10, 2.0 ** -30
    r = Rules(bsq, mask, 100, 0.5, eps_k)
    r.open(r.run)
    iterate(r, [1] * nrhs, 1.0)
    rows = check(exe, tmp_path, r)
    assert rows[a][:2] == (1, 11) and rows[b][:2] == (1, 31)
    assert all(rows[k][:2] == (1, 21) for k in bits(mask) if k not in (a, b))
