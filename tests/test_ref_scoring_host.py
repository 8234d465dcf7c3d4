"""Scoring against reference labels, the host side (no GPU): DER() of the oracle equals der_from_confusion of the confusion
block the device is asked for (here built with NumPy), and the batch interfaces validate ``ref``."""
import numpy as np
import pytest

from ref_scoring_util import numpy_confusion


def _posteriors(rng, T, S, zeros):
    q = rng.gamma(0.4, size=(T, S)) + 1e-12
    if zeros and S > 1:
        q[rng.random((T, S)) < 0.3] = 0.0                  # exact zeros ...
        q[np.arange(T), rng.integers(0, S, T)] += 0.5       # ... but never a whole row of them
        q[0] = 0.0
        q[0, S - 1] = 1.0                                   # a unit vector
    return q / q.sum(1, keepdims=True)


CASES = [  # T, S, labels drawn from, labels that get no frame
    (1, 3, 1, ()),
    (129, 4, 3, ()),
    (700, 9, 6, (2,)),           # an interior empty label
    (700, 3, 7, ()),             # R > S
    (129, 2, 6, (1, 4)),         # R > S with empty labels
    (700, 14, 14, ()),
]


@pytest.mark.parametrize('zeros', [False, True])
@pytest.mark.parametrize('T,S,R,empty', CASES)
def test_der_from_confusion_equals_the_oracles_der(T, S, R, empty, zeros):
    from oracle import vbx_oracle
    from vbx_amd import der_from_confusion
    rng = np.random.default_rng(T * 31 + S * 7 + R + zeros)
    q = _posteriors(rng, T, S, zeros)
    ref = rng.integers(0, R, T)
    for e in empty:
        ref[ref == e] = R - 1
    ref[-1] = R - 1                                         # (R = max(ref) + 1 as the reference's coo_matrix infers it)
    C = numpy_confusion(q, ref)
    assert C.shape == (2, R, S)
    for e in empty:
        assert not C[:, e].any()
    for xent in (False, True):
        want = vbx_oracle.DER(q, ref, xentropy=xent)
        got = der_from_confusion(C, T, xentropy=xent)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f'xentropy={xent}')


def test_normalise_validates_ref():
    from vbx_amd.batch import _normalise, _shape_of, PER_RECORDING
    assert 'ref' in PER_RECORDING
    rec = dict(X=np.zeros((5, 3)), Phi=np.ones(3), pi=2, gamma=np.full((5, 2), 0.5))
    assert _normalise(rec, {})['ref'] is None
    assert _normalise(dict(rec, ref=None), {})['ref'] is None
    got = _normalise(dict(rec, ref=[0, 1, 1, 3, 0]), {})['ref']
    assert got.dtype == np.int32 and got.tolist() == [0, 1, 1, 3, 0]
    assert _normalise(rec, dict(ref=np.arange(5)))['ref'].tolist() == [0, 1, 2, 3, 4]     # as a shared default
    with pytest.raises(ValueError, match='5 frames'):
        _normalise(dict(rec, ref=[0, 1, 1]), {})
    with pytest.raises(ValueError, match='negative'):
        _normalise(dict(rec, ref=[0, 1, -1, 0, 0]), {})
    with pytest.raises(ValueError, match='at most 64'):
        _normalise(dict(rec, ref=[0, 1, 64, 0, 0]), {})
    assert _normalise(dict(rec, ref=[0, 1, 63, 0, 0]), {})['ref'].max() == 63
    with pytest.raises(ValueError, match='integer'):
        _normalise(dict(rec, ref=[0.0, 1.0, 1.0, 0.0, 0.0]), {})
    # what every rank checks of a recording another rank will run
    assert _shape_of(dict(rec, ref=[0, 1, 1, 3, 0]), {})[:2] == (5, 2)
    with pytest.raises(ValueError, match='5 frames'):
        _shape_of(dict(rec, ref=[0, 1, 1]), {})
    with pytest.raises(ValueError, match='5 frames'):
        _shape_of(rec, dict(ref=np.zeros(6, dtype=int)))


def test_sweep_validates_ref_before_the_device_is_touched():
    from vbx_amd.batch import VBx_sweep
    X = np.random.default_rng(0).standard_normal((12, 8))
    g0 = np.full((12, 3), 1 / 3)
    out = VBx_sweep(X, np.ones(8), [dict(Fa=0.2), dict(Fa=0.4)], maxIters=0, pi=3, gamma=g0, ref=np.zeros(12, dtype=int))
    assert len(out) == 2 and all(t[2] == [] for t in out)
    with pytest.raises(ValueError, match='12 frames'):
        VBx_sweep(X, np.ones(8), [dict(Fa=0.2)], maxIters=0, pi=3, gamma=g0, ref=np.zeros(11, dtype=int))
    with pytest.raises(ValueError, match='at most 64'):
        VBx_sweep(X, np.ones(8), [dict(Fa=0.2)], maxIters=0, pi=3, gamma=g0, ref=np.full(12, 70))


def test_vbx_keeps_the_host_path_where_the_device_does_not_score(monkeypatch):
    from vbx_amd.VBx import _device_labels
    ref = np.array([0, 2, 1, 1])
    assert _device_labels(ref, 4).dtype == np.int32
    assert _device_labels(ref, 4, plot=True) is None
    assert _device_labels(np.array([0, 64, 1, 1]), 4) is None           # more than 64 labels
    assert _device_labels(np.array([0, 63, 1, 1]), 4) is not None
    monkeypatch.setenv('VBX_AMD_REF_SCORING', 'host')
    assert _device_labels(ref, 4) is None
