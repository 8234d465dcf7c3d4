"""A numpy referee for the device average linkage (vbx_amd/csrc/vbx_ahc.hpp, vbx_scores_linkage_average): test
infrastructure, no GPU.

  rounds_model      what the default device form does, restated in plain float64: rounds of reciprocal nearest
                    neighbours from 256 clusters on, down to 48 live clusters or three stalled rounds, then SciPy's
                    nearest-neighbour chain on what is left, then finish_linkage's stable sort and union-find
  exact_heights     the mean pairwise distance of the two clusters of every merge, summed in np.longdouble from the
                    ORIGINAL matrix: the high-precision reference, independent of any update order
  check_dendrogram  the assertions the host and the GPU tests share
  builders          the crafted inputs: seeded, each a symmetric float64 similarity matrix (or the x-vectors of one)
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'driver_split3.npz')
U = 2.0 ** -53                                               # unit roundoff of float64


# ---- the model ------------------------------------------------------------------------------------------------------
def average_update(fa, da, fb, db):
    """(n_a d_a + n_b d_b) / (n_a + n_b), every operation rounded on its own (numpy never fuses a multiply-add)"""
    return (fa * da + fb * db) / (fa + fb)


def swapped_update(fa, da, fb, db):
    """faulty model (a): the two sizes swapped"""
    return (fb * da + fa * db) / (fa + fb)


def _argmin(row, tie):
    """index of the minimum of row: the lowest among equals (the device's rule), or the highest (faulty model (b))"""
    return int(row.argmin()) if tie == 'low' else len(row) - 1 - int(row[::-1].argmin())


def finish_linkage(n, merges):
    """(a, b, d) merges in any order that respects the tree -> SciPy's Z: stable sort by height, union-find labels"""
    order = sorted(range(n - 1), key=lambda k: merges[k][2])
    parent = list(range(2 * n - 1))
    members = [1] * (2 * n - 1)

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root

    Z = np.empty((n - 1, 4))
    for k, o in enumerate(order):
        a, b, d = merges[o]
        ra, rb = find(a), find(b)
        Z[k] = [min(ra, rb), max(ra, rb), d, members[ra] + members[rb]]
        parent[ra] = parent[rb] = n + k
        members[n + k] = members[ra] + members[rb]
    return Z


def rounds_model(S, rounds_from=256, stop=48, update=average_update, tie='low', chain_too=True, stats=None):
    """Z and the per-round log [(pairs, live_before), ...] of the default device linkage on the similarities S.

    D = -S with +inf on the diagonal.  A round: nearest live neighbour per row (lowest index among equals), the reciprocal
    pairs (a < b) in index order, row b <- update (rnn_rows), then the two entries of every live row that is not dying
    (rnn_cols), between two merged rows the row of the smaller index wins (rnn_canon), sizes, and the stall rule
    pairs * 64 < T - done with `done` taken before the round.  `update` and `tie` exist for the faulty models;
    chain_too=False returns (None, log) after the rounds; stats, a dict, receives the longest chain ('max_chain') and the
    clusters handed to the chain ('chain_clusters')."""
    S = np.asarray(S, dtype=np.float64)
    T = len(S)
    D = -S
    np.fill_diagonal(D, np.inf)
    size = np.ones(T, dtype=np.int64)
    merges, log = [], []
    done = stalled = 0
    if T >= rounds_from:
        while T - done > stop and stalled < 3:
            live = size > 0
            idx = np.nonzero(live)[0]
            Dm = np.where(live[None, :], D[idx], np.inf)
            nn = np.full(T, -1)
            nn[idx] = Dm.argmin(1) if tie == 'low' else T - 1 - Dm[:, ::-1].argmin(1)
            A = np.array([i for i in idx if nn[i] > i and nn[nn[i]] == i], dtype=np.int64)
            if len(A) == 0:                                   # (cannot happen with the lowest-index rule)
                break
            B = nn[A]
            log.append((len(A), T - done))
            merges.extend((int(a), int(b), float(D[a, b])) for a, b in zip(A, B))
            na, nb = size[A].astype(np.float64), size[B].astype(np.float64)
            # rnn_rows: row b over every live column but a and b
            mask = np.repeat(live[None, :], len(A), 0)
            mask[np.arange(len(A)), A] = False
            mask[np.arange(len(A)), B] = False
            with np.errstate(invalid='ignore'):               # (masked entries hold +inf)
                new = update(na[:, None], D[A], nb[:, None], D[B])
            D[B] = np.where(mask, new, D[B])
            # rnn_cols: entries (x, b) of every live row x that is not dying, its own pair left out
            dying = np.zeros(T, dtype=bool)
            dying[A] = True
            X = np.nonzero(live & ~dying)[0]
            with np.errstate(invalid='ignore'):
                new = update(na[None, :], D[np.ix_(X, A)], nb[None, :], D[np.ix_(X, B)])
            D[np.ix_(X, B)] = np.where(X[:, None] != B[None, :], new, D[np.ix_(X, B)])
            # rnn_canon: between two merged rows the row of the smaller index wins
            Bs = np.sort(B)
            sub = D[np.ix_(Bs, Bs)]
            iu = np.triu_indices(len(Bs), 1)
            sub[iu[1], iu[0]] = sub[iu]
            D[np.ix_(Bs, Bs)] = sub
            size[B] += size[A]
            size[A] = 0
            stalled = stalled + 1 if len(A) * 64 < T - done else 0
            done += len(A)
    # SciPy's nearest-neighbour chain on what is left, compacted in order
    keep = np.nonzero(size > 0)[0]
    if stats is not None:
        stats.update(chain_clusters=len(keep), max_chain=0)
    if not chain_too:
        return None, log
    Dc = D[np.ix_(keep, keep)].copy()
    sz = size[keep].copy()
    chain = []
    for _ in range(len(keep) - 1):
        if not chain:
            chain = [int(np.nonzero(sz > 0)[0][0])]
        while True:
            x = chain[-1]
            row = np.where(sz > 0, Dc[x], np.inf)
            y, cur = (chain[-2], row[chain[-2]]) if len(chain) > 1 else (-1, np.inf)
            i = _argmin(row, tie)
            if row[i] < cur:                                  # (the previous element of the chain wins ties)
                y, cur = i, row[i]
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        if stats is not None:
            stats['max_chain'] = max(stats['max_chain'], len(chain))
        del chain[-2:]
        a, b = min(x, y), max(x, y)
        merges.append((int(keep[a]), int(keep[b]), float(cur)))
        m = sz > 0
        m[a] = m[b] = False
        v = update(float(sz[a]), Dc[a, m], float(sz[b]), Dc[b, m])
        Dc[b, m] = v
        Dc[m, b] = v
        sz[b] += sz[a]
        sz[a] = 0
    return finish_linkage(T, merges), log


# ---- the high-precision reference ---------------------------------------------------------------------------------------
def exact_heights(S, Z):
    """for every row of Z the mean pairwise distance (-S) of the two merged clusters, in np.longdouble"""
    S = np.asarray(S, dtype=np.float64)
    n = len(S)
    members = {}
    h = np.empty(n - 1, dtype=np.longdouble)
    for k in range(n - 1):
        a, b = int(Z[k, 0]), int(Z[k, 1])
        A = members.pop(a) if a >= n else np.array([a])
        B = members.pop(b) if b >= n else np.array([b])
        h[k] = -np.sum(S[np.ix_(A, B)], dtype=np.longdouble) / np.longdouble(len(A) * len(B))
        members[n + k] = np.concatenate([A, B])
    return h


def node_depths(Z):
    """height of every node of the tree above its deepest leaf (a merge of two leaves: 1)"""
    n = len(Z) + 1
    depth = np.zeros(2 * n - 1, dtype=np.int64)
    for k in range(n - 1):
        depth[n + k] = 1 + max(depth[int(Z[k, 0])], depth[int(Z[k, 1])])
    return depth[n:]


def ulps(d, d_ref):
    """largest |d - d_ref| in units of the last place of d_ref"""
    return float(np.max(np.abs(d - d_ref) / np.spacing(np.abs(d_ref))))


def exact_error(S, Z):
    """(largest |height - exact| over the bound 4 u depth max|S|, the same in ulp of the exact height)"""
    S = np.asarray(S, dtype=np.float64)
    he = exact_heights(S, Z)
    err = np.abs(Z[:, 2].astype(np.longdouble) - he)
    bound = 4 * U * node_depths(Z) * np.abs(S).max()
    return float(np.max(err / bound)), float(np.max(err / np.spacing(np.abs(he.astype(np.float64)))))


def same_partition(a, b):
    a, b = np.asarray(a).tolist(), np.asarray(b).tolist()
    return len(set(zip(a, b))) == len(set(a)) == len(set(b))


def check_valid(Z, T):
    """assertion 1: Z is a dendrogram of T leaves"""
    assert Z.shape == (T - 1, 4)
    assert np.all(np.diff(Z[:, 2]) >= 0), 'heights decrease'
    assert Z[-1, 3] == T
    kids = Z[:, :2].astype(np.int64)
    assert np.array_equal(kids, Z[:, :2]) and kids.min() >= 0
    assert np.all(kids < (T + np.arange(T - 1))[:, None]), 'a child that is not older than its parent'
    assert len(np.unique(kids)) == 2 * (T - 1), 'a node merged twice'
    size = np.concatenate([np.ones(T), Z[:, 3]])
    assert np.array_equal(size[kids[:, 0]] + size[kids[:, 1]], Z[:, 3]), 'sizes do not add up'


def check_heights(smax, Z, Z_ref, label=''):
    """assertion 3: |d - d_ref| <= max(16 ulp(d_ref), 1e-15 max|S|); the largest difference in ulp"""
    worst = ulps(Z[:, 2], Z_ref[:, 2])
    tol = np.maximum(16 * np.spacing(np.abs(Z_ref[:, 2])), 1e-15 * smax)
    bad = np.abs(Z[:, 2] - Z_ref[:, 2]) > tol
    assert not bad.any(), (label, 'heights', worst, np.argwhere(bad)[:3].tolist())
    return worst


def check_dendrogram(S, Z, Z_ref=None, distinct=True, label=''):
    """The shared assertions on a linkage matrix Z of the similarities S (the bits the linkage saw).

    1. Z is a dendrogram: shape, non-decreasing heights, sizes add up, children older than parents.
    2. (Z_ref, distinct heights) columns 0, 1, 3 are Z_ref's; the same flat clusters at the 0.2, 0.5, 0.8, 0.95 and 0.99
       quantiles of the heights, through _capi.fcluster_distance.
    3. (Z_ref) heights: |d - d_ref| <= max(16 ulp(d_ref), 1e-15 max|S|) -- 16 ulp is the bound the rounds form has always
       been held to; the floor covers heights near zero, where positive and negative distances cancel, scaled by the matrix.
    4. (distinct heights) |d - exact| <= 4 u depth_k max|S| with u = 2^-53 and depth_k the height of node k in the tree: an
       update is a convex combination of two heights, so it amplifies no error and adds at most four roundings (two
       products, a sum, a quotient) relative to the largest entry.  Z_ref is held to the same bound: if the reference alone
       exceeds it, the input is wrong, not the bound.
    Returns the measured figures."""
    S = np.asarray(S, dtype=np.float64)
    T = len(S)
    smax = np.abs(S).max()
    check_valid(Z, T)
    out = {}
    if Z_ref is not None:
        check_valid(Z_ref, T)
        if distinct:
            from vbx_amd import _capi
            same = Z[:, [0, 1, 3]] == Z_ref[:, [0, 1, 3]]
            assert same.all(), (label, 'another tree', np.argwhere(~same)[:3].tolist())
            for t in np.quantile(Z_ref[:, 2], [0.2, 0.5, 0.8, 0.95, 0.99]):
                assert same_partition(_capi.fcluster_distance(Z, float(t)), _capi.fcluster_distance(Z_ref, float(t))), (label, t)
        out['ulp_vs_ref'] = check_heights(smax, Z, Z_ref, label)
    if distinct:
        out['exact_over_bound'], out['exact_ulp'] = exact_error(S, Z)
        if Z_ref is not None:
            out['ref_exact_over_bound'], out['ref_exact_ulp'] = exact_error(S, Z_ref)
            assert out['ref_exact_over_bound'] <= 1.0, (label, 'the reference misses the bound: the input is wrong', out)
        assert out['exact_over_bound'] <= 1.0, (label, 'heights against the exact means', out)
    print(f'{label} T={T}: ' + ' '.join(f'{k}={v:.3g}' for k, v in out.items()))
    return out


# ---- the inputs -------------------------------------------------------------------------------------------------------------
def cosine(x):
    """cos_similarity of diarization_lib.py in numpy.  The products are summed in np.longdouble and rounded once: numpy
    multiplies such matrices with its own loops, so the bits do not depend on the BLAS at hand, and (i, j) and (j, i) take
    the same products in the same order -- symmetric to the last bit."""
    x = np.asarray(x, dtype=np.float64)
    xn = (x / (np.sqrt((x * x).sum(1, keepdims=True)) + 1e-32)).astype(np.longdouble)
    return (xn @ xn.T).astype(np.float64)


def example_xvectors(n):
    """the first n x-vectors of the example recording"""
    return np.load(GOLD)['xvecs'][:n].astype(np.float64)


def random_xvectors(n, D=16):
    """one seeded stream: its first 256 rows are the input of 256, the n rows after them the input of any other size"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((256, D))
    return x if n == 256 else rng.standard_normal((n, D))


def speaker_xvectors(n, noise, D=32):
    """clustered speakers: 5-7 centres, tight (noise 0.05) or like real x-vectors (0.35)"""
    rng = np.random.default_rng(2000 + n)
    k = 5 + n % 3
    centres = rng.standard_normal((k, D))
    return centres[rng.integers(0, k, n)] + noise * rng.standard_normal((n, D))


def line(p):
    """similarities of points on a line: S = -|p_i - p_j|"""
    p = np.asarray(p, dtype=np.float64)
    return -np.abs(p[:, None] - p[None, :])


def perfect_pairing(n):
    """p_i = sum_b bit_b(i) 3^b + jitter: every cluster of 2^k neighbours has its sibling as reciprocal nearest neighbour,
    so every round merges half of what is alive (n a multiple of the 2^k in question)"""
    i = np.arange(n)
    p = np.zeros(n)
    for b in range(13):
        p += ((i >> b) & 1) * 3.0 ** b
    return line(p + 1e-3 * np.random.default_rng(3000 + n).uniform(-1, 1, n))


def growing_staircase(n):
    """gaps 1 + 1e-3 i: every point's nearest neighbour is the left-hand one, ONE reciprocal pair per round -> the rounds stall"""
    return line(np.cumsum(1.0 + 1e-3 * np.arange(n)))


def shrinking_staircase(n):
    """gaps 2 - step i, all positive and distinct: every point's nearest neighbour is the right-hand one, so the chain that
    starts at point 0 grows to length n before its first merge"""
    step = 1e-3 if n <= 1000 else 1e-4
    return line(np.cumsum(2.0 - step * np.arange(n)))


def constant(n, c=0.25):
    return np.full((n, n), c)


# Two inputs with exact ties whose resolution SciPy fixes, for the faulty tie rule (on distinct distances no tie rule is
# ever consulted, so no such input can tell one rule from another).
def tied_staircase(n):
    """gaps 1 + 0.5 (i // 3): every third point sits exactly half-way between its neighbours"""
    return line(np.cumsum(1.0 + 0.5 * (np.arange(n) // 3)))


def random_with_a_tie(n):
    """random cosine similarities with ONE planted tie: points n/3 and 2n/3 are both the nearest neighbour of point 0, closer
    to it than any other two points are to each other.  SciPy's chain starts at point 0 with no predecessor, so the lowest
    index wins: (0, n/3) merge first."""
    S = cosine(random_xvectors(n))
    top = (S - np.eye(n)).max()
    for k in (n // 3, 2 * n // 3):
        S[0, k] = S[k, 0] = (1.0 + top) / 2
    return S
