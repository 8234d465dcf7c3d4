"""CPU-only: the automatic choice of VBX_OPT_STREAM_LOADS is a rule on byte counts (vbx_stream_loads_auto): non-temporal loads
of rho where ONE copy of the x-vectors that iterate together is larger than the 256 MiB Infinity Cache."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


def test_auto_rule_is_pinned_to_byte_counts():
    from vbx_amd import _capi
    lib = _capi.load()
    auto = lambda nbytes: int(lib.vbx_stream_loads_auto(int(nbytes)))
    rho = lambda n_rec, T, Dp=128, rsize=4: n_rec * T * Dp * rsize
    assert auto(256 * MIB) == 0 and auto(256 * MIB + 1) == 1          # the Infinity Cache itself still fits
    assert auto(0) == 0
    assert auto(rho(64, 10000)) == 1                                    # the headline batch: 328 MB per copy
    assert auto(rho(1, 10000)) == 0 and auto(rho(4, 10000)) == 0 and auto(rho(8, 10000)) == 0
    assert auto(rho(1, 200000)) == 0                                    # the sweep over one shared rho counts it once: 102 MB
    assert auto(rho(32, 10000)) == 0 and auto(rho(53, 10000)) == 1      # 164 MB / 271 MB
    assert auto(rho(64, 10000, rsize=8)) == 1


def test_option_constants_match_the_header():
    from vbx_amd import _capi
    text = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    val = lambda name: int(re.search(rf'#define {name} (\d+)', text).group(1))
    assert _capi.OPT_STREAM_LOADS == val('VBX_OPT_STREAM_LOADS')
    assert (_capi.STREAM_LOADS_AUTO, _capi.STREAM_LOADS_ON, _capi.STREAM_LOADS_OFF) == \
        (val('VBX_STREAM_LOADS_AUTO'), val('VBX_STREAM_LOADS_ON'), val('VBX_STREAM_LOADS_OFF'))
    assert _capi.STREAM_LOADS_NAMES == {'auto': 0, 'on': 1, 'off': 2}
