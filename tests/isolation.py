"""What a call may read, stated without a device (numpy only).

The C ABI promises that a batched entry point neither reads nor writes the systems outside `mask`.  A kernel that loads such a system and
multiplies it by zero, that fills the surplus rows of a tile from the stride padding, or that loads the lhs a ZERO piece is about to clear,
gives the right numbers as long as those bytes are finite.  This module makes them not finite:

  poisoned(buf, keep)     a copy of a host operand with every byte outside the element mask `keep` set to 0xFF -- the pattern of the
                          "malloc_poison" tuning key, a NaN in complex<double>, complex<float> and complex<half>
  band / unband           an operand inside a larger image with GUARD = 4096 poisoned bytes in front of it and behind it, so that a
                          whole-line or whole-tile over-read lands in memory the test owns; 4096 is a multiple of 16, so the operand
                          keeps its 16-byte alignment, or the misalignment by `lead` elements a row asks for
  *_reads                 one function per entry family: which elements of each operand the call may read and which it writes, from
                          what the route tables carry (entry, mask, nrhs, stride, pieces, flags)
  check_isolation         runs a call on the clean and on the poisoned operands through one `execute` callable and compares bytes

The read-set rules:
  * the segments of systems outside `mask` are not read, in every vector operand;
  * stride padding is not read, nor the leading element of a misaligned operand;
  * the rhs parity that no selected piece takes as a source is not read (a clover or shift bit of parity p reads rhs_p, a hop bit of
    parity p reads rhs_{1-p}; a bit whose field is absent selects nothing);
  * an lhs half is read only if a piece accumulates into it: not where ZERO clears it, not where no piece touches it;
  * a pure scratch operand is not read anywhere;
  * a buffer with two roles (lhs is rhs) is poisoned only where no role reads it;
  * entries without a mask treat every system as active; the one-system epilogue entry reads `system` alone.
Never poisoned: the matrices, the gauge field, the null vectors, and the rhs rows a partial slab launch does not need.
"""
import numpy as np

POISON = 0xFF
GUARD = 4096

# include/qmg_hip.h
P_CLOVER_E, P_CLOVER_O = 1 << 0, 1 << 1
P_EO, P_OE = 0xF << 2, 0xF << 6
P_SHIFT_E, P_SHIFT_O = 1 << 10, 1 << 11
P_ZERO_E, P_ZERO_O = 1 << 12, 1 << 13


# ---------------------------------------------------------------- bytes
def poisoned(buf, keep):
    """a copy of `buf` with every byte of the elements outside the boolean mask `keep` set to 0xFF"""
    a = np.ascontiguousarray(buf).copy()
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    assert keep.size == a.size, (keep.size, a.size)
    a.reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize)[~keep] = POISON
    return a


def band(a, lead=0):
    """(image, offset): the bytes of `a` behind GUARD poisoned bytes and `lead` poisoned elements, with GUARD poisoned bytes behind it"""
    a = np.ascontiguousarray(a)
    offset = GUARD + lead * a.dtype.itemsize
    image = np.full(offset + a.nbytes + GUARD, POISON, dtype=np.uint8)
    image[offset:offset + a.nbytes] = a.reshape(-1).view(np.uint8)
    return image, offset


def unband(image, offset, like):
    """the operand inside an image, in the dtype and size of `like`"""
    return image[offset:offset + like.nbytes].copy().view(like.dtype)


def byte_mask(elements, itemsize):
    return np.repeat(np.asarray(elements, dtype=bool).reshape(-1), itemsize)


class Operand:
    """One buffer of a call: its clean host contents, the elements the call may read, the elements it writes (None: read-only), and the
    leading elements of a deliberate misalignment."""

    def __init__(self, clean, reads, writes=None, lead=0):
        self.clean = np.ascontiguousarray(clean)
        n = self.clean.size
        self.reads = np.broadcast_to(np.asarray(reads, dtype=bool), (n,)).copy()
        self.writes = np.zeros(n, dtype=bool) if writes is None else np.broadcast_to(np.asarray(writes, dtype=bool), (n,)).copy()
        self.lead = lead

    def poisoned_bytes(self):
        return int(np.count_nonzero(~self.reads)) * self.clean.dtype.itemsize

    def merged(self, other):
        """the same buffer in a second role: read where either role reads, written where either writes"""
        assert other.clean.tobytes() == self.clean.tobytes() and other.lead == self.lead
        return Operand(self.clean, self.reads | other.reads, self.writes | other.writes, self.lead)


class Leak(AssertionError):
    pass


def check_isolation(operands, execute, served=True):
    """Run `execute` on the clean and on the poisoned operands and hold the two runs to each other.

    operands: {name: Operand}.  execute({name: (image, offset)}) -> ({name: image after the call}, scalars) where scalars is a bytes-like of
    the reductions of the ACTIVE systems (b"" if none), or raises if the call is refused (served = False expects that of both runs: `execute`
    then returns the images it found after the refusal).

      * every element the call writes has the same bytes in both runs;
      * every other byte of every image of the poisoned run -- read-only operands, padding, frozen systems, the guard bands -- is what was
        uploaded: 0xFF wherever the rule poisons;
      * the scalars have the same bits.
    Returns {name: poisoned bytes inside the operand}.
    """
    runs = []
    for poison in (False, True):
        images = {}
        for name, op in operands.items():
            images[name] = band(poisoned(op.clean, op.reads) if poison else op.clean, op.lead)
        before = {name: im.copy() for name, (im, _) in images.items()}
        after, scalars = execute(images)
        runs.append((before, after, bytes(scalars)))
    (_, clean_after, clean_scalars), (before, after, scalars) = runs
    for name, op in operands.items():
        item = op.clean.dtype.itemsize
        offset = GUARD + op.lead * item
        written = np.zeros(before[name].size, dtype=bool)
        if served:
            written[offset:offset + op.clean.nbytes] = byte_mask(op.writes, item)
        got, want = after[name], clean_after[name]
        if not np.array_equal(got[written], want[written]):
            bad = np.flatnonzero(written & (got != want))
            raise Leak("%s: element %d of the output differs between the clean and the poisoned run (%d bytes differ): the call read what it must not"
                       % (name, (int(bad[0]) - offset) // item, bad.size))
        if not np.array_equal(got[~written], before[name][~written]):
            bad = np.flatnonzero(~written & (got != before[name]))
            raise Leak("%s: byte %d (operand starts at %d, %d bytes) was written outside the elements the call writes" % (name, int(bad[0]), offset, op.clean.nbytes))
    if scalars != clean_scalars:
        raise Leak("the reductions differ between the clean and the poisoned run")
    return {name: op.poisoned_bytes() for name, op in operands.items()}


# ---------------------------------------------------------------- read-set rules
def active(mask, nrhs):
    return [k for k in range(nrhs) if (mask >> k) & 1]


def source_parities(pieces, has_clover=True, has_hopping=True):
    """[even read, odd read]: the rhs parities some selected piece takes as a source"""
    out = [False, False]
    for p in (0, 1):
        if (has_clover and pieces & (P_CLOVER_E << p)) or pieces & (P_SHIFT_E << p):
            out[p] = True
        if has_hopping and pieces & (P_EO << (4 * p)):
            out[1 - p] = True
    return out


def lhs_parities(pieces, has_clover=True, has_hopping=True):
    """([even written, odd written], [even read, odd read]) of lhs: a parity is written if a piece with its field present or a ZERO bit
    selects it; it is read only if a piece accumulates into it (any of its bits set, its ZERO bit not)"""
    writes, reads = [False, False], [False, False]
    for p in (0, 1):
        work = bool((has_clover and pieces & (P_CLOVER_E << p)) or pieces & (P_SHIFT_E << p) or (has_hopping and pieces & (P_EO << (4 * p))))
        named = bool(pieces & ((P_CLOVER_E | P_SHIFT_E) << p | (P_EO << (4 * p))))
        zero = bool(pieces & (P_ZERO_E << p))
        writes[p] = work or zero
        reads[p] = named and not zero
    return writes, reads


def _segments(nrhs, stride, size, systems, per_system):
    """a mask over nrhs * stride elements: `per_system` (size elements) on each of `systems`, False elsewhere (padding, frozen systems)"""
    m = np.zeros(nrhs * stride, dtype=bool)
    for k in systems:
        m[k * stride:k * stride + size] = per_system
    return m


def _halves(size, flags2):
    h = np.zeros(size, dtype=bool)
    h[:size // 2], h[size // 2:] = flags2[0], flags2[1]
    return h


def stencil_reads(entry, dims, nrhs, stride, mask, pieces, flags="", has_clover=True, has_hopping=True):
    """{role: (reads, writes)} over nrhs * stride elements for the stored-stencil entries (qmg_stencil_apply*, the h16 and epilogue forms).
    entry: apply | masked | h16 | norm2 | epi.  Roles: rhs, lhs, and for the epilogue other / dotv where the flags pass them."""
    Lx, Ly, nc = dims
    size = Lx * Ly * nc
    fl = flags.split()
    act = active(mask, nrhs)
    if entry in ("apply", "norm2"):
        act = list(range(nrhs))             # no mask: every system
    elif entry == "epi":
        act = act[:1]                       # one system per launch
    if Lx == 1 and Ly == 1:                 # the corner form: one even site, the shift term alone
        src = np.full(size, bool(pieces & P_SHIFT_E))
        wr = np.full(size, bool(pieces & (P_ZERO_E | P_ZERO_O | P_SHIFT_E)))
        rd = np.full(size, bool(pieces & P_SHIFT_E) and not pieces & (P_ZERO_E | P_ZERO_O))
    else:
        src = _halves(size, source_parities(pieces, has_clover, has_hopping))
        w2, r2 = lhs_parities(pieces, has_clover, has_hopping)
        wr, rd = _halves(size, w2), _halves(size, r2)
    seg = lambda per: _segments(nrhs, stride, size, act, per)
    none = np.zeros(nrhs * stride, dtype=bool)
    out = {"rhs": (seg(src), none), "lhs": (seg(rd), seg(wr))}
    if entry == "epi":                      # out = other_scale other + acc_scale acc on the processed parities; the dots run over them
        for role in ("other", "dots"):
            if role in fl:
                out["dotv" if role == "dots" else role] = (seg(wr), none)
    return out


def wilson_reads(entry, dims, nrhs, stride, hstride, mask, pieces, flags=""):
    """{role: (reads, writes)} for qmg_wilson_apply_direct / qmg_wilson_hops_direct and their _epi forms on an Lx x Ly slab with nc = 2.
    Roles: rhs, lhs, lo, hi (over nrhs * hstride; only where the flags name a slab), other, dotv."""
    Lx, Ly = dims
    size = 2 * Lx * Ly
    fl = flags.split()
    hops = entry.startswith("hops")
    act = active(mask, nrhs)
    src = source_parities(pieces, has_clover=not hops)
    w2, r2 = lhs_parities(pieces, has_clover=not hops)
    rows = None
    for f in fl:
        if f.startswith("slab"):
            rows = int(f[4])
    row_on = np.zeros((2, Ly, Lx), dtype=bool)
    row_on[:, {None: slice(None), 0: slice(None), 1: slice(1, Ly - 1), 2: [0, Ly - 1]}[rows]] = True
    row_on = row_on.reshape(-1)
    seg = lambda per: _segments(nrhs, stride, size, act, per)
    none = np.zeros(nrhs * stride, dtype=bool)
    wr, rd = _halves(size, w2) & row_on, _halves(size, r2) & row_on
    out = {"rhs": (seg(_halves(size, src)), none), "lhs": (seg(rd), seg(wr))}
    if rows is not None and "nohalos" not in fl:
        hop_src = [bool(pieces & (P_EO << (4 * (1 - q)))) for q in (0, 1)]       # a halo row is rhs data: read by the hops alone
        halo = _segments(nrhs, hstride, 2 * Lx, act, _halves(2 * Lx, hop_src) & (rows != 1))
        out["lo"] = out["hi"] = (halo, np.zeros(nrhs * hstride, dtype=bool))
    if entry.endswith("_epi"):
        if "other" in fl or "aliaslhs" in fl:
            out["other"] = (seg(wr), none)
        if {"dots", "dotsrhs", "dotsother"} & set(fl):
            out["dotv"] = (seg(wr), none)
    return out


def transfer_reads(op, fsize, csize, nrhs, fstride, cstride, mask):
    """{role: (reads, writes)} for the batched restrict / prolong: both accumulate, so the output of an active system is read"""
    act = active(mask, nrhs)
    fine, coarse = _segments(nrhs, fstride, fsize, act, True), _segments(nrhs, cstride, csize, act, True)
    if op == "restrict":
        return {"fine": (fine, np.zeros_like(fine)), "coarse": (coarse, coarse.copy())}
    return {"coarse": (coarse, np.zeros_like(coarse)), "fine": (fine, fine.copy())}


def dwf_reads(entry, n, nrhs, stride, mask, pieces=0, parity=0):
    """{role: (reads, writes)} for the domain-wall entries on 5-d vectors of n elements (even half first).
    entry: direct (qmg_dwf_apply_direct: the stencil rule, clover, hops and shift all present) | inv5 (kernel I: overwrites the parities its
    clover bits name from the same parity of rhs) | hops (kernel K: the stencil rule on the hop and ZERO bits) | schur (reads rhs_p, writes
    lhs_p and tmp_{1-p}; lhs is overwritten and tmp is pure scratch: neither is read)."""
    act = active(mask, nrhs)
    seg = lambda per: _segments(nrhs, stride, n, act, per)
    none = np.zeros(nrhs * stride, dtype=bool)
    if entry == "inv5":
        on = [bool(pieces & (P_CLOVER_E << p)) for p in (0, 1)]
        return {"rhs": (seg(_halves(n, on)), none), "lhs": (none, seg(_halves(n, on)))}
    if entry == "schur":
        p_half, o_half = _halves(n, [parity == 0, parity == 1]), _halves(n, [parity == 1, parity == 0])
        return {"rhs": (seg(p_half), none), "lhs": (none, seg(p_half)), "tmp": (none, seg(o_half))}
    if entry == "hops":
        pieces &= P_EO | P_OE | P_ZERO_E | P_ZERO_O
    src = source_parities(pieces)
    w2, r2 = lhs_parities(pieces)
    return {"rhs": (seg(_halves(n, src)), none), "lhs": (seg(_halves(n, r2)), seg(_halves(n, w2)))}


def meas_reads(entry, n5, n4, nsys, stride5, stride4):
    """{role: (reads, writes)} for the dwf_meas entries with nsys systems: the gaps between systems are never read.
    wall_source writes psi5 from eta4; wall_project writes q4 from psi5; slice_norms reads psi5."""
    five, four = _segments(nsys, stride5, n5, range(nsys), True), _segments(nsys, stride4, n4, range(nsys), True)
    if entry == "wall_source":
        return {"eta4": (four, np.zeros_like(four)), "psi5": (np.zeros_like(five), five)}
    if entry == "wall_project":
        return {"psi5": (five, np.zeros_like(five)), "q4": (np.zeros_like(four), four)}
    return {"psi5": (five, np.zeros_like(five))}


def operands_of(roles, clean, aliases=(), leads=None):
    """{name: Operand} from a rule's {role: (reads, writes)} and {role: clean host array}; aliases: (role, role) pairs that share one
    buffer -- the pair becomes one operand under the first name, poisoned only where neither role reads"""
    leads = leads or {}
    ops = {r: Operand(clean[r], rw[0], rw[1], leads.get(r, 0)) for r, rw in roles.items()}
    for a, b in aliases:
        ops[a] = ops[a].merged(ops.pop(b))
    return ops
