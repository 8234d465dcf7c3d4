"""Shape tables of the ragged-batch tests of the x-vector network (tests/test_gpu_xvector_ragged.py) and the host test that
keeps them honest (tests/test_xvector_ragged_host.py).  Importing this module touches neither a GPU nor the golden files.

A kernel case is (H, widths, Cin, Cout / BN): a ragged batch of windows of H rows and widths[b] columns.  A window gives
Ho Wo[b] output rows; the rows of all windows, end to end, are cut into tiles of BM rows by the kernel, and into slabs of 32
rows by its wavefronts.  What a case is there for depends on where the windows' boundaries fall in that cut, so the table is
a function of the stride and of BM, and check_cases() states the conditions it has to meet."""
import resnet_shapes as rs

# every instantiation of both convolution kernels
INSTANTIATIONS = [(ks, s, bn, bm) for ks, s in rs.KS_STRIDE for bn, bm in rs.TILES]

STEM_WIDTHS = [3, 1, 18, 2]                               # the stem's and the pooling's ragged batch
NETWORK_LENGTHS = [1, 2, 9, 10, 11, 23, 143, 144, 145, 167]


def out_rows(H, widths, stride):
    """Output rows of every window of a case."""
    return [rs.rn_out(H, stride) * rs.rn_out(w, stride) for w in widths]


def spans(H, widths, stride):
    """[(first output row, one past the last)] of every window in the concatenation."""
    out, m = [], 0
    for r in out_rows(H, widths, stride):
        out.append((m, m + r))
        m += r
    return out


def kernel_cases(stride, bm):
    """The cases of the instantiations with this stride and BM.  At H = 1 a window of width w gives rn_out(w, stride) rows:
    `w(r)` is the odd and `w(r, True)` the even width that gives r rows at stride 2 (both r at stride 1)."""
    def w(r, even=False):
        return r if stride == 1 else (2 * r if even else 2 * r - 1)
    r2 = rs.rn_out(2, stride)                              # rows of a window of width 2
    return [
        # tile 0 = windows of bm - 5, 2 and 3 rows (the middle one inside the tile, a neighbour either side; the third ends
        # on the tile's edge); a window over tiles 1 .. 3; widths 1 and 2; a last one that fills tile 3: M = 4 BM
        (1, [w(bm - 5), w(2, True), w(3), w(2 * bm + 7, True), 1, 2, w(bm - 8 - r2)], 16, 1),
        # M = BM + 1; the first window crosses the slab edge at row 32
        (1, [w(40, True), w(17), w(bm - 56)], 32, 2),
        # M = BM - 1: one partial tile; the second window crosses row 32
        (1, [w(20), w(25, True), w(bm - 46)], 48, 1),
        # rows that wrap: a row of a window ends where the next begins, inside a tile
        (2, [1, 2, 3, 18, 5, 4], 32, 2),
        (8, [3, 1, 18, 2, 7], 64, 1),
    ]


def check_cases(stride, bm, cases):
    """Raises AssertionError unless the cases of one (stride, BM) meet every condition the kernel tests rely on."""
    edge = inside = three = slab = False
    residues, small, widths_seen = set(), False, set()
    for H, widths, cin, cf in cases:
        assert H in (1, 2, 8) and 16 <= cin <= 64 and cin % 16 == 0 and cf in (1, 2) and min(widths) >= 1
        sp = spans(H, widths, stride)
        M = sp[-1][1]
        residues.add(M % bm)
        small |= M < bm
        widths_seen |= set(widths)
        for b, (m0, m1) in enumerate(sp):
            edge |= m1 % bm == 0 and m1 < M
            inside |= 0 < b < len(sp) - 1 and m0 // bm == (m1 - 1) // bm and m0 % bm != 0 and m1 % bm != 0
            three |= (m1 - 1) // bm - m0 // bm >= 2
            slab |= m0 % 32 != 0 and m0 // 32 != (m1 - 1) // 32
    assert edge, 'no window ends exactly on a BM edge'
    assert inside, 'no window lies inside one tile with a neighbour on either side'
    assert three, 'no window spans three tiles'
    assert {1, 2} <= widths_seen, 'widths 1 and 2 must occur'
    assert stride == 1 or ({w % 2 for w in widths_seen} == {0, 1}), 'odd and even widths must occur at stride 2'
    assert slab, 'no window straddles a 32-row slab'
    assert {0, 1, bm - 1} <= residues, ('M mod BM', sorted(residues))
    assert small, 'no case with M < BM'
