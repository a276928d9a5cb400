"""CPU emulation of the point kernels (hsds_amd/csrc/points.h, run thread by thread by
tests/emu/points_emu.cpp) against the numpy model of the hsds_points_* contract
(include/hsds_amd.h): random points over datasets whose chunks do not divide the extent,
every element size and compound variant, the point counts around one wavefront, duplicate
writes, missing chunks, dst_index permutations, outputs 4 bytes off a 16-byte boundary, and
the unsigned out-of-extent test.  Test infrastructure only."""
import numpy as np
import pytest

import points_cases as pc


@pytest.fixture(scope="module")
def emu():
    return pc.Emu()


def _located(emu, c):
    chunk, eoff, nbad = emu.locate(c["dims"], c["layout"], c["dt"].itemsize, c["pts"])
    mc, me, mb = pc.locate_model(c["dims"], c["layout"], c["dt"].itemsize, c["pts"])
    assert nbad == mb == 0 and (chunk == mc).all() and (eoff == me).all()
    return chunk, eoff


CASES = [(gi, di, n) for gi in range(len(pc.GEOMS)) for di in range(len(pc.DTYPES))
         for n in (pc.COUNTS if (gi, di) in ((1, 2), (0, 4), (2, 6)) else [pc.COUNTS[1 + (gi + di) % 5]])]


@pytest.mark.parametrize("gi,di,n", CASES)
def test_random_points(emu, gi, di, n):
    dims, layout = pc.GEOMS[gi]
    dt = pc.DTYPES[di]
    c = pc.random_case(1000 * gi + 10 * di + n, dims, layout, dt, n)
    which, eoff = _located(emu, c)
    E, segs = c["E"], c["segs"]
    out0 = np.full(n * E, 0x5A, np.uint8)
    # contiguous output, on and 4 bytes off a 16-byte boundary; fill pattern and zero fill
    for shift, fill in ((0, c["fill"]), (4, None), (4, c["fill"])):
        got = emu.gather(c["arena"], c["slot"], which, eoff, segs, dt.itemsize, E, fill, out0, shift=shift,
                         nthreads=1 + n % 7)
        assert (got == pc.gather_model(c["arena"], c["slot"], which, eoff, segs, E, fill, out0)).all(), shift
    # a permutation of a larger response: the other elements stay as they were
    rng = np.random.default_rng(n)
    dst_index = rng.permutation(n + 5)[:n]
    big = rng.integers(0, 256, (n + 5) * E, dtype=np.uint8)
    for shift in (0, 4):
        got = emu.gather(c["arena"], c["slot"], which, eoff, segs, dt.itemsize, E, c["fill"], big, dst_index=dst_index,
                         shift=shift)
        assert (got == pc.gather_model(c["arena"], c["slot"], which, eoff, segs, E, c["fill"], big, dst_index)).all()
    # duplicate writes: the last request position wins; missing chunks are skipped
    order = pc.sort_order(which, eoff, c["chunk_bytes"])
    got = emu.scatter(c["arena"], c["slot"], which, eoff, order, segs, dt.itemsize, E, c["vals"], nthreads=1 + n % 5)
    assert (got == pc.scatter_model(c["arena"], c["slot"], which, eoff, segs, E, c["vals"])).all()


@pytest.mark.parametrize("fields", [["a"], ["a", "b"], ["b", "c"], ["c"], ["a", "c"]])
@pytest.mark.parametrize("n", [1, 65])
def test_field_subsets(emu, fields, n):
    """named fields only: a read packs them, a write leaves the other fields alone"""
    dims, layout = pc.GEOMS[1]
    c = pc.random_case(len(fields) * 100 + n + ord(fields[0][0]), dims, layout, pc.ABC, n, fields=fields)
    which, eoff = _located(emu, c)
    E, segs = c["E"], c["segs"]
    assert E == sum(pc.ABC.fields[f][0].itemsize for f in fields)
    out0 = np.full(n * E, 0x33, np.uint8)
    for shift in (0, 4):
        got = emu.gather(c["arena"], c["slot"], which, eoff, segs, 12, E, c["fill"], out0, shift=shift)
        assert (got == pc.gather_model(c["arena"], c["slot"], which, eoff, segs, E, c["fill"], out0)).all()
    order = pc.sort_order(which, eoff, c["chunk_bytes"])
    got = emu.scatter(c["arena"], c["slot"], which, eoff, order, segs, 12, E, c["vals"])
    assert (got == pc.scatter_model(c["arena"], c["slot"], which, eoff, segs, E, c["vals"])).all()
    # the model itself against numpy field assignment on one resident chunk
    arr = np.zeros(layout, pc.ABC)
    arr.view(np.uint8).reshape(-1)[:] = np.arange(arr.nbytes) % 251
    sdt = pc.subset_dtype(pc.ABC, fields)
    pts = np.array([[0, 0], [6, 4], [3, 2], [6, 4]], np.uint64)
    vals = np.zeros(4, sdt)
    vals.view(np.uint8)[:] = np.arange(vals.nbytes) % 13 + 65
    want = arr.copy()
    for p, v in zip(pts, vals):
        for f in fields:
            want[f][tuple(int(x) for x in p)] = v[f]
    _, e2, _ = emu.locate(layout, layout, 12, pts)
    got = emu.scatter(arr.view(np.uint8).reshape(-1), [0], None, e2, pc.sort_order(None, e2, arr.nbytes), segs, 12, E,
                      vals.view(np.uint8))
    assert (got == want.view(np.uint8).reshape(-1)).all()


def test_padding_bytes(emu):
    """an align=True compound: a read gives zeros in the padding, a write leaves the chunk's"""
    dt = pc.DTYPES[7]
    assert dt.itemsize == 24
    c = pc.random_case(5, (20, 11), (7, 5), dt, 65, missing=False)
    assert c["segs"] == [(0, 0, 1), (8, 8, 10)]          # u | v and w (neighbours merge), padding left out
    which, eoff = _located(emu, c)
    mask = np.tile(pc.field_mask(dt), 65)
    got = emu.gather(c["arena"], c["slot"], which, eoff, c["segs"], 24, 24, None, np.full(65 * 24, 0xEE, np.uint8),
                     shift=4)
    assert not got[~mask].any()
    order = pc.sort_order(which, eoff, c["chunk_bytes"])
    after = emu.scatter(c["arena"], c["slot"], which, eoff, order, c["segs"], 24, 24, c["vals"])
    changed = np.nonzero(after != c["arena"])[0]
    amask = np.zeros(c["arena"].size, bool)
    for k, e in zip(which, eoff):
        amask[c["slot"][k] + e:c["slot"][k] + e + 24] = pc.field_mask(dt)
    assert amask[changed].all()


def test_out_of_extent_is_unsigned(emu):
    dims, layout = (20, 11), (7, 5)
    pts = np.array([[0, 0], [19, 10], [20, 0], [0, 11], [2 ** 63, 0], [3, 2 ** 64 - 1], [2 ** 63 + 5, 2 ** 63 + 3],
                    [2 ** 32 + 3, 1], [7, 5]], np.uint64)
    chunk, eoff, nbad = emu.locate(dims, layout, 8, pts)
    assert nbad == 6
    assert list(chunk) == [0, 8, -1, -1, -1, -1, -1, -1, 4]
    assert list(eoff[[0, 1, 8]]) == [0, (5 * 5 + 0) * 8, 0]
    mc, me, mb = pc.locate_model(dims, layout, 8, pts)
    assert mb == 6 and (mc == chunk).all() and (me == eoff).all()


def test_extents_beyond_32_bits(emu):
    dims, layout = (2 ** 40, 2 ** 33 + 7), (2 ** 20 + 3, 2 ** 32 + 1)
    pts = np.array([[2 ** 40 - 1, 2 ** 33 + 6], [12345678901, 2 ** 32], [5, 2 ** 32 + 1], [2 ** 40, 0]], np.uint64)
    chunk, eoff, nbad = emu.locate(dims, layout, 1, pts)
    mc, me, mb = pc.locate_model(dims, layout, 1, pts)
    assert nbad == mb == 1 and (mc == chunk).all() and (me == eoff).all()


def test_argument_checks(emu):
    a = np.zeros(64, np.uint8)
    e = np.zeros(1, np.int64)
    ok = [(0, 0, 4)]
    assert isinstance(emu.gather(a, [0], None, e, ok, 4, 4, None, np.zeros(4, np.uint8)), np.ndarray)
    bad = [[(0, 0, 5)],                       # past the output element
           [(2, 0, 4)],                       # past the chunk element
           [(0, 2, 2), (0, 0, 2)],            # not sorted by out_off
           [(0, 0, 3), (0, 2, 2)],            # overlap
           [(0, 0, 0)],                       # empty segment
           [(0, k, 1) for k in range(17)]]    # too many
    for segs in bad:
        E = 32 if len(segs) > 16 else 4
        assert emu.gather(a, [0], None, e, segs, E, E, None, np.zeros(E, np.uint8)) == -6, segs
        assert emu.scatter(a, [0], None, e, None, segs, E, E, np.zeros(E, np.uint8)) == -6, segs
