"""Shape tables shared by the x-vector network's kernel tests (tests/test_gpu_resnet_kernels.py), its network tests
(tests/test_gpu_xvector.py) and the host test that keeps them honest (tests/test_xvector_host.py).  Importing this module
touches neither a GPU nor the golden files; conv_classes() calls vbx_resnet_conv_tile, which is host code."""
from vbx_amd import _capi, xvector

# the instantiations of resnet_conv_kernel<KS, S, BN, BM>
KS_STRIDE = [(1, 1), (1, 2), (3, 1), (3, 2)]
TILES = [(128, 64), (128, 128), (64, 64), (64, 128), (32, 128)]
RESIDUES = (0, 1, 31, 32, 33, 63)                         # M mod BM of the forced-tile cases, and BM - 1


def rn_out(n, stride):
    return (n - 1) // stride + 1


def _geometry(bm, residue):
    """(n, Ho, Wo) with n Ho Wo = residue mod bm, two to four tiles, and images that end inside tiles: the first in a
    fixed order of small odd and even factors (an image of one row, Ho = 1, only where nothing else factors)."""
    for rows in ((5, 3, 7, 4, 6, 2, 9, 8, 11), (1,)):
        for n in (3, 5, 2, 7, 4, 6):
            for ho in rows:
                for wo in range(2, 4 * bm):
                    m = n * ho * wo
                    if m % bm == residue and bm < m <= 4 * bm and (ho * wo) % bm != 0:
                        return n, ho, wo
    raise AssertionError((bm, residue))


def _forced_cases():
    """(ks, stride, bn, bm, n, H, W): every instantiation at every residue of M mod BM, and at one partial tile in all
    (n = 3, Ho x Wo = 3 x 5: M = 45).  At stride 2, H and W alternate between the odd and the even size that gives Ho, Wo."""
    out = []
    for ks, stride in KS_STRIDE:
        for bn, bm in TILES:
            geoms = [_geometry(bm, r) for r in sorted(set(RESIDUES + (bm - 1,)))] + [(3, 3, 5)]
            for k, (n, ho, wo) in enumerate(geoms):
                h = ho if stride == 1 else 2 * ho - (k & 1)
                w = wo if stride == 1 else 2 * wo - ((k >> 1) & 1)
                assert rn_out(h, stride) == ho and rn_out(w, stride) == wo
                out.append((ks, stride, bn, bm, n, h, w))
    return out


FORCED_CASES = _forced_cases()

# (n, T) of the network runs of tests/test_gpu_xvector.py::test_production_shapes
NETWORK_RUNS = [(37, 144), (3, 85), (9, 113), (15, 137), (29, 141), (58, 141)]
# ... and of its other tests, beside the per-length groups of the fixture windows and the CLI's batches, which
# fixture_runs() derives from the fixture: test_batch_invariance, test_large_batch_past_2_gib, test_nan_stays_in_its_window
# and test_device_inputs_give_the_same_bits
OTHER_RUNS = [(1, 144), (128, 144), (512, 144), (15, 20), (1, 20), (4, 144), (3, 144), (2, 26)]
CLI_BATCH = 16                                            # test_cli_with_a_checkpoint_reproduces_predict_py


def fixture_runs(win_rec, win_len, seg_len=144):
    """(n, T) of test_fixture_windows_match_the_reference (all windows of one length at once) and of the CLI test (per
    recording: full windows CLI_BATCH at a time, every other length in one batch)."""
    win_rec, win_len = [int(r) for r in win_rec], [int(t) for t in win_len]
    runs = {(win_len.count(t), t) for t in set(win_len)}
    for rec in set(win_rec):
        lens = [t for r, t in zip(win_rec, win_len) if r == rec]
        for t in set(lens):
            n = lens.count(t)
            if t == seg_len:
                runs |= {(min(CLI_BATCH, n - b0), t) for b0 in range(0, n, CLI_BATCH)}
            else:
                runs.add((n, t))
    return sorted(runs)


def network_convs(T, embed_dim=256):
    """(ks, stride, Cin, Cout, H, W) of every convolution of one run at T frames, in network order (the stem, a kernel of
    its own, left out), and the embedding as the 1 x 1 convolution it runs as."""
    out = [(ks, stride, cin, cout, H, W) for (_, _, ks, stride, cin, cout), H, W in xvector.walk(T)]
    return out + [(1, 1, xvector.POOL_DIM, (embed_dim + 31) // 32 * 32, 1, 1)]


_tile_cache = {}


def conv_tile(M, Cout):
    """(BN, BM) the library's dispatcher picks (vbx_resnet_conv_tile)."""
    key = (M, Cout)
    if key not in _tile_cache:
        _tile_cache[key] = _capi.resnet_conv_tile(M, Cout)
    return _tile_cache[key]


def conv_classes(n, T):
    """{(ks, stride, BN, BM, last tile partial)} of every convolution of one run of n windows of T frames."""
    out = set()
    for ks, stride, _, cout, h, w in network_convs(T):
        M = n * rn_out(h, stride) * rn_out(w, stride)
        bn, bm = conv_tile(M, cout)
        out.add((ks, stride, bn, bm, M % bm != 0))
    return out


def layer_cases(embedding=False):
    """(ks, stride, Cin, Cout, H, W, n): every distinct convolution of the network at the W that T = 141 and 144 give at
    its depth, at the smallest n of the domain for every tile the dispatcher can pick for it; and (embedding) the embedding."""
    out = []
    domain = list(range(1, 129)) + [192, 256, 384, 512]
    for layer in sorted({c for T in (141, 144) for c in network_convs(T)[:-1]}):
        ks, stride, cin, cout, H, W = layer
        hw = rn_out(H, stride) * rn_out(W, stride)
        first = {}
        for n in domain:
            first.setdefault(conv_tile(n * hw, cout), n)
        out += [layer + (n,) for n in first.values()]
    return out + [(1, 1, xvector.POOL_DIM, 256, 1, 1, n) for n in (1, 3, 37) if embedding]
