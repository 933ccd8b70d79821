"""Every restrict / prolong kernel of csrc/qmg_transfer.hip and csrc/qmg_transfer_mfma.hip against an independent reference, one row per
route.

ROUTES is the table: entry point (op x storage), fd -> cd, nrhs, mask and the plan the row is meant to hit, in qmg_transfer_plan's
terms.  A row first asserts that the library routes the request as the row says (every pass of it), so a retune that moves a kernel
out from under its row fails here, and tests/test_host_transfer_plan.py fails when a plan exists that no row expects.  Then the entry
point runs on padded strides, masks with holes and non-zero initial contents, and EVERY active system is compared with
transfer_numpy's long-double reference (inputs rounded to complex<float> first where the storage is narrow):
  whole vector   relative L2 < 1e-13 (fp64 results) or TOL32_ROUND = 3e-7 (complex<float> results)
  elementwise    |got - want| <= (nel + 1) 2^-50 S, plus 2^-23 |want| for complex<float> results (transfer_numpy.elementwise_bound)
Frozen systems and all padding must come back bit-identical, and a second run of the same call must give the same bytes (every kernel
here has one writer per output and a fixed summation order).
"""
import importlib

import numpy as np
import pytest

import coordspace as cs
import transfer_numpy as tn

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

TOL64 = 1e-13
TOL32_ROUND = 3e-7    # fp64 arithmetic, one fp32 rounding of the result (test_gpu_f32.py)
FPAD, CPAD = 6, 4     # padding elements behind every fine / coarse vector (even: a complex<float> system stays 16-byte aligned)


# ---- plans, as qmg_transfer_plan writes them: (family, KB, NV, MT, CR, nchunk, small, W)
def MFMA(MT, CR, nchunk, small):
    return (qmg.XF_BRESTRICT_MFMA, 8, 0, MT, CR, nchunk, small, 0)


def SMALL(KB, NVT):
    return (qmg.XF_BRESTRICT_SMALL, KB, NVT, 0, 0, 0, 0, 0)


def TILE(KB):
    return (qmg.XF_BRESTRICT_TILE, KB, 0, 0, 0, 0, 0, 0)


def PTILE(KB, NVB):
    return (qmg.XF_BPROLONG_TILE, KB, NVB, 0, 0, 0, 0, 0)


def ONE_R(W):
    return (qmg.XF_RESTRICT, 1, 0, 0, 0, 0, 0, W)


def ONE_P(W):
    return (qmg.XF_PROLONG, 1, 0, 0, 0, 0, 0, W)


GENERIC = (qmg.XF_RESTRICT_GENERIC, 1, 0, 0, 0, 0, 0, 1)
NV32_R = (qmg.XF_RESTRICT_NV32, 1, 0, 0, 0, 0, 0, 2)
NV32_P = (qmg.XF_PROLONG_NV32, 1, 0, 0, 0, 0, 0, 2)
REFUSED = (qmg.XF_UNSUPPORTED, 0, 0, 0, 0, 0, 0, 0)

R, P = "restrict", "prolong"
M13 = 0b1011111101110111   # 13 of 16
M12 = 0b0111101101111011   # 12 of 16
M9 = 0b0000101011111011    # 9 of 12

# (op, storage, fd, cd, nrhs, mask, plans of the passes[, "misaligned"])
ROUTES = [
    # ---- the matrix-core restrict (complex<float>, 5-8 systems, fnc <= 2, 16 <= nvec <= 32)
    (R, "c32", (8, 8, 2), (2, 2, 16), 5, 0b11111, [MFMA(1, 8, 1, 1)]),             # MT = 1, one chunk, ragged workgroup (cLx = 2), pairs < BLOCK
    (R, "c32", (8, 8, 2), (2, 2, 16), 8, 0xFF, [MFMA(1, 8, 1, 1)]),
    (R, "c32", (24, 8, 2), (6, 2, 24), 8, 0b10110111, [MFMA(2, 8, 1, 1)]),         # MT = 2, a full and a ragged workgroup (cLx = 6)
    (R, "c32", (8, 8, 2), (2, 2, 20), 6, 0b101111, [MFMA(2, 8, 1, 1)]),            # nvec = 20: the zeroed rows of the second tile
    (R, "c32", (8, 8, 2), (2, 2, 32), 5, 0b11111, [MFMA(2, 8, 1, 1)]),
    (R, "c32", (32, 16, 2), (4, 2, 24), 8, 0xFF, [MFMA(2, 4, 4, 1)]),              # 8x8 blocks: CR = 4, four chunks
    (R, "c32", (32, 16, 2), (4, 2, 16), 8, 0b11110111, [MFMA(1, 8, 2, 0)]),        # CR = 8, two chunks, pairs = 256: the strided staging
    (R, "c32", (8, 8, 1), (4, 2, 16), 5, 0b11111, [MFMA(1, 8, 1, 1)]),             # fnc = 1, 2x4 blocks: G = 1, eight d-groups
    (R, "c32", (4, 2, 2), (2, 2, 16), 6, 0b111011, [MFMA(1, 2, 1, 1)]),            # 2x1 blocks of nc = 2: one MFMA step per site
    (R, "c32", (4, 4, 1), (2, 2, 16), 5, 0b11111, [MFMA(1, 4, 1, 1)]),             # 2x2 blocks of nc = 1
    (R, "c32", (16, 16, 2), (2, 2, 16), 5, 0b11111, [MFMA(1, 8, 2, 1)]),           # 8x8 blocks on two coarse columns: two chunks, pairs = 128
    (R, "c32", (32, 16, 1), (4, 2, 16), 7, 0b1111111, [MFMA(1, 16, 1, 0)]),        # 8x8 blocks of nc = 1: CR = 16, pairs = 256
    (R, "c32", (16, 16, 1), (2, 2, 16), 5, 0b11111, [MFMA(1, 16, 1, 1)]),
    (R, "c32", (4, 2, 2), (2, 2, 20), 5, 0b11111, [MFMA(2, 2, 1, 1)]),
    (R, "c32", (4, 4, 1), (2, 2, 24), 7, 0b1101111, [MFMA(2, 4, 1, 1)]),
    (R, "c32", (32, 16, 2), (4, 2, 20), 5, 0b11111, [MFMA(2, 8, 2, 0)]),
    (R, "c32", (16, 16, 2), (2, 2, 20), 8, 0xFF, [MFMA(2, 8, 2, 1)]),
    (R, "c32", (32, 16, 1), (4, 2, 20), 5, 0b11111, [MFMA(2, 16, 1, 0)]),
    (R, "c32", (16, 16, 1), (2, 2, 20), 5, 0b11111, [MFMA(2, 16, 1, 1)]),
    # ---- declined by the matrix cores
    (R, "c32", (8, 4, 1), (4, 4, 16), 5, 0b11111, [SMALL(8, 16)]),                 # no tile: 2x1 blocks of nc = 1
    (R, "c32", (8, 8, 2), (2, 2, 40), 5, 0b11111, [TILE(8)]),                      # nvec = 40
    # ---- two passes
    (R, "c32", (8, 8, 2), (2, 2, 16), 16, M13, [MFMA(1, 8, 1, 1), MFMA(1, 8, 1, 1)]),   # 8 + 5
    (R, "c32", (8, 8, 2), (2, 2, 16), 16, M12, [MFMA(1, 8, 1, 1), SMALL(4, 16)]),       # 8 + 4
    (R, "c32", (8, 8, 2), (2, 2, 16), 12, M9, [MFMA(1, 8, 1, 1), SMALL(2, 16)]),        # 8 + 1: one live slot
    (R, "c64", (8, 8, 2), (2, 2, 8), 16, M13, [SMALL(8, 8), SMALL(8, 8)]),
    (P, "c32", (8, 8, 2), (2, 2, 16), 12, M9, [PTILE(8, 12), PTILE(2, 4)]),
    (P, "c64", (8, 8, 2), (2, 2, 6), 16, M12, [PTILE(8, 4), PTILE(4, 4)]),
    # ---- k_brestrict_small: KB x NVT, nvec not a multiple of 16 / KB (6, 13, 20), nel = 32 and nel < 32
    (R, "c64", (8, 4, 2), (4, 2, 6), 2, 0b11, [SMALL(2, 8)]),
    (R, "c64", (8, 8, 2), (2, 2, 13), 3, 0b101, [SMALL(2, 16)]),
    (R, "c64", (8, 4, 2), (4, 2, 20), 2, 0b11, [SMALL(2, 24)]),
    (R, "c64", (8, 8, 2), (2, 2, 8), 3, 0b111, [SMALL(4, 8)]),
    (R, "c64", (8, 4, 2), (4, 2, 13), 5, 0b11011, [SMALL(4, 16)]),
    (R, "c64", (8, 8, 2), (2, 2, 24), 4, 0b1011, [SMALL(4, 24)]),
    (R, "c64", (8, 8, 2), (2, 2, 6), 8, 0b10110111, [SMALL(8, 8)]),
    (R, "c64", (8, 8, 2), (2, 2, 16), 6, 0b111111, [SMALL(8, 16)]),
    (R, "c64", (8, 4, 2), (4, 2, 20), 6, 0b111111, [SMALL(8, 24)]),
    (R, "c32", (8, 8, 2), (2, 2, 6), 2, 0b11, [SMALL(2, 8)]),
    (R, "c32", (8, 4, 2), (4, 2, 13), 2, 0b11, [SMALL(2, 16)]),
    (R, "c32", (8, 8, 2), (2, 2, 20), 3, 0b110, [SMALL(2, 24)]),
    (R, "c32", (8, 4, 2), (4, 2, 6), 4, 0b1111, [SMALL(4, 8)]),
    (R, "c32", (8, 8, 2), (2, 2, 13), 3, 0b111, [SMALL(4, 16)]),
    (R, "c32", (8, 4, 2), (4, 2, 24), 4, 0b1111, [SMALL(4, 24)]),
    (R, "c32", (8, 4, 2), (4, 2, 8), 6, 0b111111, [SMALL(8, 8)]),
    (R, "c32", (8, 8, 2), (2, 2, 13), 8, 0b10110111, [SMALL(8, 16)]),
    (R, "c32", (4, 4, 3), (2, 2, 20), 6, 0b111111, [SMALL(8, 24)]),                # fnc = 3: declined by the matrix cores
    # ---- k_brestrict_tile: nel = 128, and nel = 48 (no multiple of 32)
    (R, "c64", (8, 8, 8), (2, 2, 12), 2, 0b11, [TILE(2)]),
    (R, "c64", (8, 8, 3), (2, 2, 6), 4, 0b1111, [TILE(4)]),
    (R, "c64", (8, 8, 8), (2, 2, 12), 8, 0b11101111, [TILE(8)]),
    (R, "c32", (8, 8, 3), (2, 2, 6), 2, 0b11, [TILE(2)]),
    (R, "c32", (8, 8, 8), (2, 2, 12), 5, 0b11011, [TILE(4)]),
    (R, "c32", (8, 8, 3), (2, 2, 6), 7, 0b1111111, [TILE(8)]),
    # ---- k_bprolong_tile<float, 8, 12>: 12 + 12, 12 + 4, 12 + 2 scalar, 12 + 1
    (P, "c32", (8, 8, 2), (2, 2, 24), 5, 0b11111, [PTILE(8, 12)]),
    (P, "c32", (8, 8, 2), (2, 2, 16), 8, 0xFF, [PTILE(8, 12)]),
    (P, "c32", (8, 8, 2), (2, 2, 14), 6, 0b101111, [PTILE(8, 12)]),
    (P, "c32", (8, 8, 2), (2, 2, 13), 5, 0b11111, [PTILE(8, 12)]),
    (P, "c32", (24, 8, 2), (6, 2, 24), 8, 0xFF, [PTILE(8, 12)]),
    (P, "c32", (24, 4, 4), (6, 2, 13), 8, 0b10110111, [PTILE(8, 12)]),             # tiles of 4 sites on 6 columns: a ragged last tile
    # ---- k_bprolong_tile<T, KB, 4>
    (P, "c64", (8, 8, 2), (2, 2, 6), 2, 0b11, [PTILE(2, 4)]),
    (P, "c64", (24, 8, 2), (6, 2, 24), 3, 0b111, [PTILE(4, 4)]),
    (P, "c64", (8, 8, 2), (2, 2, 8), 8, 0b10110111, [PTILE(8, 4)]),
    (P, "c64", (24, 4, 4), (6, 2, 6), 3, 0b101, [PTILE(2, 4)]),                    # ragged last tile
    (P, "c32", (8, 8, 2), (2, 2, 24), 2, 0b11, [PTILE(2, 4)]),
    (P, "c32", (8, 8, 2), (2, 2, 6), 3, 0b111, [PTILE(4, 4)]),
    (P, "c32", (24, 8, 2), (6, 2, 8), 6, 0b111111, [PTILE(8, 4)]),
    (P, "c32", (24, 4, 4), (6, 2, 8), 6, 0b111111, [PTILE(8, 4)]),                 # ragged last tile
    # ---- an odd block width in a batch: system by system
    (R, "c64", (12, 8, 2), (4, 2, 4), 4, 0b1101, [GENERIC]),
    (R, "c32", (12, 8, 2), (4, 2, 4), 4, 0b1101, [GENERIC]),
    (P, "c64", (12, 8, 2), (4, 2, 4), 4, 0b1101, [ONE_P(1)]),
    (P, "c32", (12, 8, 2), (4, 2, 4), 4, 0b1101, [ONE_P(2)]),
    # ---- the one-system kernels: 16-byte packs, one element per lane from an odd fnc, and from a misaligned complex<float> pointer
    (R, "c64", (8, 8, 2), (2, 2, 8), 1, 0b1, [ONE_R(1)]),
    (P, "c64", (8, 8, 2), (2, 2, 8), 1, 0b1, [ONE_P(1)]),
    (R, "c32", (8, 8, 2), (2, 2, 8), 1, 0b1, [ONE_R(2)]),
    (P, "c32", (8, 8, 2), (2, 2, 8), 1, 0b1, [ONE_P(2)]),
    (R, "c32", (8, 8, 3), (2, 2, 6), 1, 0b1, [ONE_R(1)]),
    (P, "c32", (8, 8, 3), (2, 2, 6), 1, 0b1, [ONE_P(1)]),
    (R, "c32", (8, 8, 2), (2, 2, 8), 2, 0b10, [ONE_R(1)], "misaligned"),
    (P, "c32", (8, 8, 2), (2, 2, 8), 2, 0b10, [ONE_P(1)], "misaligned"),
    # ---- complex<float> null vectors under complex<double> vectors, and their refusals
    (R, "nv32", (8, 8, 2), (2, 2, 8), 1, 0b1, [NV32_R]),
    (P, "nv32", (8, 8, 2), (2, 2, 8), 1, 0b1, [NV32_P]),
    (R, "nv32", (8, 8, 2), (2, 2, 8), 4, 0b1011, [NV32_R]),
    (P, "nv32", (8, 8, 2), (2, 2, 8), 4, 0b1011, [NV32_P]),
    (P, "nv32", (12, 8, 2), (4, 2, 4), 3, 0b111, [NV32_P]),                        # (the prolong takes an odd block width)
    (R, "nv32", (12, 8, 2), (4, 2, 4), 3, 0b111, [REFUSED]),                       # odd block width
    (R, "nv32", (8, 8, 3), (2, 2, 6), 1, 0b1, [REFUSED]),                          # odd fnc
    (P, "nv32", (8, 8, 3), (2, 2, 6), 1, 0b1, [REFUSED]),
    (R, "nv32", (8, 8, 2), (2, 2, 8), 1, 0b1, [REFUSED], "misaligned"),            # null vectors not 16-byte aligned
    (P, "nv32", (8, 8, 2), (2, 2, 8), 1, 0b1, [REFUSED], "misaligned"),
    # ======== past the caps of the grid (qmg_transfer_plan exports no grid: the row counts are held against the launch code's caps here)
    # ---- k_restrict: grid.y = min(cLy, 65535) blocks walk the coarse rows; cLy = 65538, so three blocks take a second row cy = 65535 .. 65537
    (R, "c64", (4, 131076, 2), (2, 65538, 2), 1, 0b1, [ONE_R(1)]),
    (R, "c32", (4, 131076, 2), (2, 65538, 2), 1, 0b1, [ONE_R(2)]),
    (R, "nv32", (4, 131076, 2), (2, 65538, 2), 1, 0b1, [NV32_R]),
    # ---- k_prolong: grid.y = min(2 fLy, 65535) blocks walk the fine rows row = parity fLy + y; 2 fLy = 65544, so nine blocks take a second
    #      row 65535 .. 65543 (parity 1, y = 32763 .. 32771)
    (P, "c64", (4, 32772, 2), (2, 16386, 4), 1, 0b1, [ONE_P(1)]),
    (P, "c32", (4, 32772, 2), (2, 16386, 4), 1, 0b1, [ONE_P(2)]),
    (P, "nv32", (4, 32772, 2), (2, 16386, 4), 1, 0b1, [NV32_P]),
    # ---- k_bprolong_tile and k_brestrict_mfma: grid.y = min(cLy, 65535) blocks walk the coarse rows and restage their LDS tile per row;
    #      cLy = 65538 again (the matrix-core restrict: 16 null vectors of 1 048 608 complex<float>, 134 MB)
    (P, "c64", (4, 131076, 2), (2, 65538, 2), 2, 0b11, [PTILE(2, 4)]),
    (R, "c32", (4, 131076, 2), (2, 65538, 16), 5, 0b11111, [MFMA(1, 4, 1, 1)]),
    # ---- k_prolong: grid.x = min(blocks of a row, 1024) blocks of 256 lanes walk the fhr fnc / W = 10924 * 24 = 262 176 packs of a fine
    #      row, so the first 32 lanes take a second pack 262 144 .. 262 175
    (P, "c64", (21848, 2, 24), (10924, 2, 2), 1, 0b1, [ONE_P(1)]),
]
GRID_Y_MAX, GRID_X_LANES = 65535, 1024 * 256      # the caps of the launch code (csrc/qmg_transfer.hip, csrc/qmg_transfer_mfma.hip)
# which cap a geometry is about: "tall" coarse rows, "tallfine" fine (parity, y) rows, "wide" the packs of a fine row
CAPPED = {((4, 131076, 2), (2, 65538, 2)): "tall", ((4, 131076, 2), (2, 65538, 16)): "tall", ((4, 32772, 2), (2, 16386, 4)): "tallfine",
          ((21848, 2, 24), (10924, 2, 2)): "wide"}


def walked_second(row):
    """the mask over one output vector of what a block, or a lane, reaches on its second trip; None for a row that is not about a cap"""
    op, _, fd, cd = row[:4]
    tag = CAPPED.get((fd, cd), "")
    if tag == "tall":             # coarse rows cy >= 65535: of the coarse vector (restrict), or the fine rows of their blocks (prolong)
        assert cd[1] > GRID_Y_MAX
        dims, y0 = (cd, GRID_Y_MAX) if op == R else (fd, GRID_Y_MAX * (fd[1] // cd[1]))
        grid = np.zeros(dims, dtype=bool)
        grid[:, y0:] = True
        return tn._to_eo(grid, *dims)
    if tag == "tallfine":         # fine rows in storage order, row = parity fLy + y >= 65535
        assert 2 * fd[1] > GRID_Y_MAX
        m = np.zeros((2 * fd[1], fd[0] // 2 * fd[2]), dtype=bool)
        m[GRID_Y_MAX:] = True
        return m.reshape(-1)
    if tag == "wide":             # the packs (one element each in complex<double>) of every fine row beyond grid.x * block
        assert fd[0] // 2 * fd[2] > GRID_X_LANES
        m = np.zeros((2 * fd[1], fd[0] // 2 * fd[2]), dtype=bool)
        m[:, GRID_X_LANES:] = True
        return m.reshape(-1)
    return None


def route_id(row):
    op, storage, fd, cd, nrhs, mask = row[:6]
    return "%s-%s-%dx%dx%d-%dx%dx%d-n%d-%x%s" % ((op, storage) + fd + cd + (nrhs, mask, "-mis" if len(row) > 7 else ""))


def active(mask, nrhs):
    return [k for k in range(nrhs) if (mask >> k) & 1]


def planned(row):
    """what qmg_transfer_plan answers for the row's request"""
    op, storage, fd, cd, nrhs, mask = row[:6]
    return qmg.transfer_plan(qmg.XFER_RESTRICT if op == R else qmg.XFER_PROLONG, qmg.C32 if storage == "c32" else qmg.C64, storage == "nv32", cd[2], fd, cd,
                             len(active(mask, nrhs)), aligned16=len(row) == 7)


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    qmg.sync()


def r32(a):
    return np.ascontiguousarray(a, dtype=np.complex64).astype(np.complex128)


class Dev:
    """A host array on the device, behind one leading element when the row asks for a pointer that is not 16-byte aligned."""

    def __init__(self, a, dtype, shift):
        self.shift = shift
        self.arr = qmg.DeviceArray.from_host(np.concatenate([np.zeros(shift, dtype=dtype), np.ascontiguousarray(a, dtype=dtype)]))
        self.ptr = self.arr.offset(shift)

    def host(self):
        return self.arr.to_host()[self.shift:]


def call(row, dn, dfine, dcoarse, fstride, cstride):
    op, storage, fd, cd, nrhs, mask = row[:6]
    nvec = cd[2]
    if storage == "nv32":
        if op == R:
            qmg.restrict_batch_nv32(dn.ptr, nvec, dfine.ptr, dcoarse.ptr, fd, cd, nrhs, fstride, cstride, mask)
        else:
            qmg.prolong_batch_nv32(dn.ptr, nvec, dcoarse.ptr, dfine.ptr, fd, cd, nrhs, cstride, fstride, mask)
    else:
        dtype = qmg.C32 if storage == "c32" else qmg.C64
        if op == R:
            qmg.restrict_batch_t(dtype, dn.ptr, nvec, dfine.ptr, dcoarse.ptr, fd, cd, nrhs, fstride, cstride, mask)
        else:
            qmg.prolong_batch_t(dtype, dn.ptr, nvec, dcoarse.ptr, dfine.ptr, fd, cd, nrhs, cstride, fstride, mask)


@pytest.mark.parametrize("row", ROUTES, ids=route_id)
def test_route_against_numpy_reference(row):
    op, storage, fd, cd, nrhs, mask, plans = row[:7]
    mis = len(row) > 7
    assert planned(row) == plans
    second = walked_second(row)
    nvec = cd[2]
    fsize, csize = fd[0] * fd[1] * fd[2], cd[0] * cd[1] * cd[2]
    fstride, cstride = fsize + FPAD, csize + CPAD
    nv, fine0, coarse0 = cs.gaussian_cvec(nvec * fsize, 1), cs.gaussian_cvec(nrhs * fstride, 2), cs.gaussian_cvec(nrhs * cstride, 3)
    vdt = np.complex64 if storage == "c32" else np.complex128     # the vectors' storage
    ndt = np.complex128 if storage == "c64" else np.complex64     # the null vectors'
    if storage != "c64":
        nv = r32(nv)
    if storage == "c32":
        fine0, coarse0 = r32(fine0), r32(coarse0)
    # the misaligned pointer: the fine vector (one-system kernels), the null vectors (nv32)
    dn = Dev(nv, ndt, 1 if mis and storage == "nv32" else 0)
    fshift = 1 if mis and storage == "c32" else 0

    def run():
        dfine, dcoarse = Dev(fine0, vdt, fshift), Dev(coarse0, vdt, 0)
        call(row, dn, dfine, dcoarse, fstride, cstride)
        return (dcoarse if op == R else dfine).host()

    init, ostride, osize = (coarse0, cstride, csize) if op == R else (fine0, fstride, fsize)
    if plans == [REFUSED]:
        with pytest.raises(qmg.QmgError, match="unsupported"):
            run()
        return
    raw = run()
    got = raw.astype(np.complex128)
    untouched = np.ones(nrhs * ostride, dtype=bool)
    for i, k in enumerate(active(mask, nrhs)):
        fk, ck = fine0[k * fstride:k * fstride + fsize], coarse0[k * cstride:k * cstride + csize]
        want, S = tn.restrict(nv, fk, fd, cd, ck) if op == R else tn.prolong(nv, ck, fd, cd, fk)
        seg = slice(k * ostride, k * ostride + osize)
        untouched[seg] = False
        err = np.abs(got[seg].astype(tn.CLD) - want)
        bound = tn.elementwise_bound(op, fd, cd, S, want if storage == "c32" else None)
        l2 = float(np.linalg.norm(err) / np.linalg.norm(want))
        # (the figures DESIGN 10.6 quotes per plan: run with -s)
        print("route %s system %d plan %s %s: max err/bound %.3f, rel L2 %.3e" % (route_id(row), k, storage, plans[i // 8 if len(plans) > 1 else 0], float(np.max(err / bound)), l2))
        assert l2 < (TOL32_ROUND if storage == "c32" else TOL64), (k, l2)
        assert np.all(err <= bound), (k, int(np.argmax(err / bound)), float(np.max(err / bound)))
        if second is not None:      # what is reached on a second trip, on its own
            l2 = float(np.linalg.norm(err[second]) / np.linalg.norm(want[second]))
            assert np.any(second) and l2 < (TOL32_ROUND if storage == "c32" else TOL64), (k, "second trip", l2)
            assert np.all(err[second] <= bound[second]), (k, "second trip", float(np.max(err[second] / bound[second])))
    # frozen systems and every padding element: the initial bytes
    assert np.array_equal(got[untouched], init[untouched])
    assert run().tobytes() == raw.tobytes()
