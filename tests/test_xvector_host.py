"""The x-vector network's host side (vbx_amd/xvector.py): the synthetic checkpoint against the fixture recorded from the
unmodified predict.py + models/resnet.py (tests/golden/make_golden_resnet.py), the checkpoint checks, the BatchNorm fold and
packing, and the CLI's refusals.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from vbx_amd import xvector

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = np.load(os.path.join(REPO, 'tests', 'golden', 'resnet_cases.npz'))
F = np.load(os.path.join(REPO, 'tests', 'golden', 'fbank_cases.npz'))
SEED, E = int(R['seed']), int(R['embed_dim'])


def window(j):
    """fixture window j as the network input [64][T]"""
    name = str(F['names'][R['win_rec'][j]])
    rows = F['rows_' + name]
    s, a, n = int(R['win_seg'][j]), int(R['win_start'][j]), int(R['win_len'][j])
    r0 = int(rows[:s].sum())
    return F['fea_' + name][r0 + a:r0 + a + n].T


@pytest.fixture(scope='module')
def sd():
    return xvector.synthetic_state_dict(SEED, E)


def test_synthetic_state_dict_rebuilds_the_fixture(sd):
    # the shortest windows: the f64 forward of the rebuilt checkpoint gives the recorded referee embeddings
    for j in np.argsort(R['win_len'], kind='stable')[:3]:
        got = xvector.forward_reference(sd, window(j)[None])[0]
        ref = R['emb_f64'][j]
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.abs(R['emb_ref'][j] - ref).max() <= 2e-6 * np.abs(ref).max()   # (the reference's own f32 run)


def test_layout_and_parameter_count(sd):
    assert len(xvector.conv_specs()) == 1 + 3 * 33 + 4
    assert xvector.fold(sd).shape == (xvector.n_params(E),)
    assert 14.5e6 < xvector.n_params(256) < 15e6
    perm = xvector.pool_order()
    assert np.array_equal(np.sort(perm), np.arange(xvector.POOL_DIM))
    assert perm[1] == 8 and perm[1024] == 1 and perm[8192] == 8192                  # (h 1024 + c) <- c 8 + h


def test_checkpoint_checks(sd, tmp_path):
    import torch
    extra = dict(sd, **{'bn1.num_batches_tracked': np.array(7), 'something.else': np.zeros(3)})
    assert set(xvector.check_state_dict(extra)) == set(sd)
    bad = dict(sd)
    del bad['layer3.17.bn2.running_var']
    with pytest.raises(ValueError, match=r'layer3\.17\.bn2\.running_var'):
        xvector.check_state_dict(bad)
    bad = dict(sd, **{'layer2.0.shortcut.0.weight': np.zeros((256, 64, 1, 1), np.float32)})
    with pytest.raises(ValueError, match=r'layer2\.0\.shortcut\.0\.weight has shape \(256, 64, 1, 1\)'):
        xvector.check_state_dict(bad)
    with pytest.raises(ValueError, match="module."):
        xvector.check_state_dict({'module.' + k: v for k, v in sd.items()})
    with pytest.raises(ValueError, match='embedding.weight'):
        xvector.check_state_dict(sd, embed_dim=128)
    path = str(tmp_path / 'ck.pth')
    torch.save({'state_dict': {k: torch.from_numpy(np.asarray(v)) for k, v in extra.items()}, 'epoch': 3}, path)
    got = xvector.load_checkpoint(path)
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    with pytest.raises(ValueError, match='state_dict'):
        xvector.load_checkpoint(path)


def test_fold_and_packing_match_the_unfolded_network(sd):
    rng = np.random.default_rng(5)
    x = np.concatenate([window(j)[None] for j in np.flatnonzero(R['win_len'] == 19)[:1]] +
                       [rng.standard_normal((1, 64, 19))])
    ref = xvector.forward_reference(sd, x)
    got = xvector.forward_folded(xvector.fold(sd), E, x)
    assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max()


def test_network_runs_reach_every_reachable_convolution_class():
    """The (n, T) the GPU tests run the network at reach every class (ks, stride, BN, BM, last M-tile partial) of
    resnet_conv_kernel that predict can ask for: n <= 128 and 192 / 256 / 384 / 512 windows of 10 ... 144 frames.  The tile
    is the library's own choice (vbx_resnet_conv_tile), so a change of the dispatcher's thresholds fails here until
    resnet_shapes.NETWORK_RUNS is extended."""
    import resnet_shapes as rs
    convs = {T: [(ks, s, cout, rs.rn_out(h, s) * rs.rn_out(w, s)) for ks, s, _, cout, h, w in rs.network_convs(T)]
             for T in range(10, 145)}

    def classes(n, T):
        out = set()
        for ks, s, cout, hw in convs[T]:
            bn, bm = rs.conv_tile(n * hw, cout)
            out.add((ks, s, bn, bm, n * hw % bm != 0))
        return out

    assert classes(3, 26) == rs.conv_classes(3, 26)
    domain = set()
    for T in convs:
        for n in list(range(1, 129)) + [192, 256, 384, 512]:
            domain |= classes(n, T)
    tested = set()
    for n, T in rs.NETWORK_RUNS + rs.OTHER_RUNS + rs.fixture_runs(R['win_rec'], R['win_len']):
        tested |= classes(n, T)
    assert tested == domain, sorted(domain ^ tested)
    assert all((bn, bm) in rs.TILES for _, _, bn, bm, _ in domain)


def test_the_network_walk_is_what_it_was():
    """xvector.walk / flops and resnet_shapes.network_convs against literals recorded from the hand-written loops they replace."""
    import hashlib
    import resnet_shapes as rs
    digest = {10: 'e8a7602b07607708', 141: '34b5bc635944d6ca', 144: 'e75d2e1992ba3593'}
    for T, want in digest.items():
        convs = rs.network_convs(T)
        assert len(convs) == 104
        assert hashlib.sha256(repr(convs).encode()).hexdigest()[:16] == want, T
    convs = rs.network_convs(144)
    assert convs[0] == (1, 1, 32, 32, 64, 144) and convs[3] == (1, 1, 32, 128, 64, 144)
    assert convs[4] == (1, 1, 128, 32, 64, 144) and convs[10] == (1, 1, 128, 64, 64, 144)
    assert convs[-2] == (1, 1, 256, 1024, 8, 18) and convs[-1] == (1, 1, 16384, 256, 1, 1)
    assert rs.network_convs(10)[-2] == (1, 1, 256, 1024, 8, 2)
    assert xvector.flops(144) == {'stem': 5308416, 'layer1': 981467136, 'layer2': 1509949440, 'layer3': 7606370304,
                                  'layer4': 1189085184}
    assert xvector.flops(19) == {'stem': 700416, 'layer1': 129499136, 'layer2': 208666624, 'layer3': 1056440320,
                                 'layer4': 193986560}
    assert len(list(xvector.blocks())) == 33 and [spec for spec, _, _ in xvector.walk(144)] == xvector.conv_specs()[1:]


def test_forced_tile_table_holds_every_instantiation():
    import resnet_shapes as rs
    cases = rs.FORCED_CASES
    assert {c[:4] for c in cases} == {ks_s + t for ks_s in rs.KS_STRIDE for t in rs.TILES} and len({c[:4] for c in cases}) == 20
    for ks, s in rs.KS_STRIDE:
        for bn, bm in rs.TILES:
            ms = [n * rs.rn_out(h, s) * rs.rn_out(w, s) for k, st, b1, b2, n, h, w in cases if (k, st, b1, b2) == (ks, s, bn, bm)]
            assert {m % bm for m in ms} >= {0, 1, 31, 32, 33, 63, bm - 1}, (ks, s, bn, bm)
            assert any(m < bm for m in ms)


def test_cli_refuses_checkpoint_with_model_file():
    base = ['--in-file-list', 'l', '--in-lab-dir', 'd', '--in-wav-dir', 'd', '--out-ark-fn', 'a', '--out-seg-fn', 's']
    for extra, msg in ((['--gpus', '0', '--checkpoint', 'c.pth', '--model-file', 'm'], 'exclude each other'),
                       (['--gpus', '0', '--model', 'ResNet101', '--weights', 'w', '--checkpoint', 'c.pth'],
                        '--model/--weights are not supported'),
                       (['--gpus', '0'], '--checkpoint')):
        res = subprocess.run([sys.executable, '-m', 'vbx_amd.predict'] + base + extra, cwd=REPO, capture_output=True,
                             text=True, timeout=120)
        assert res.returncode != 0 and msg in res.stderr
