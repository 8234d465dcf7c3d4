"""The staging loads of the per-chunk kernels, as the compiler emitted them (no GPU needed).

stage_to_lds and the alpha staging of the split chunk_loglik instances exist to put every load of a staging round in
flight before the first of them is waited for.  The sources said so for a long time while the code object issued them one
round trip at a time (each behind ``s_waitcnt vmcnt(0)``), so this is held in the disassembly of the built library:

  * the NST ``global_load_dwordx4`` of chunk_post's b tile -- the loads whose registers a ``ds_write_b128`` stores before the
    first barrier -- have no full wait between the first and the last of them;
  * the alpha loads of a staging round of chunk_loglik likewise;
  * the instances keep the occupancy they are launched for and no scratch memory (kernel descriptors of the code object).

tools/loads_in_flight.py, which prints these sequences, is tested on a small synthetic listing.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))

POST_STREAM = '_ZN3vbx17chunk_post_kernelIfLi32ELb0ELb1ELb0EJNS_11StreamLoadsEEEEvNS_9BatchViewIT_EE'
POST_SPLIT = '_ZN3vbx17chunk_post_kernelIfLi32ELb0ELb1ELb0EJEEEvNS_9BatchViewIT_EE'
LOGLIK_LAT_STREAM = '_ZN3vbx19chunk_loglik_kernelIfLi32ELb1ELb1EJNS_11StreamLoadsEEEEvNS_9BatchViewIT_EE'
LOGLIK_SPLIT = '_ZN3vbx19chunk_loglik_kernelIfLi32ELb1ELb0EJEEEvNS_9BatchViewIT_EE'
NST = 4                      # 16-byte vectors of a 128 x 32 f32 tile per thread of 256
ALPHA_ROUND = 4              # ... of a staging round of alpha: 2 N-tiles x 2 K-blocks x 3 terms x 1 KB over 256 threads


def _build():
    from vbx_amd import build as hipbuild
    if not hipbuild.OBJDUMP:
        pytest.skip('llvm-objdump not available')
    assert os.path.exists(hipbuild.LIB), f'{hipbuild.LIB} is not built'
    return hipbuild


@pytest.fixture(scope='module')
def bodies():
    import loads_in_flight as lif
    return dict(lif.kernels(_build().disassemble()))


def _staged_loads(body, until_first_barrier):
    """Indices (into body) of the global_load_dwordx4 whose destination registers a later ds_write_b128 stores -- up to the
    first barrier (chunk_post: the b tile) or to the last f16 matrix instruction (chunk_loglik: the staging rounds of
    alpha; later phases reuse the registers for values that were never loaded)."""
    end = len(body)
    if not until_first_barrier:
        end = max(i for i, code in enumerate(body) if code.startswith('v_mfma_f32_16x16x32_f16')) + 1
    last_load, staged = {}, []
    for i, code in enumerate(body[:end]):
        op = code.split()[0]
        if op == 'global_load_dwordx4':
            last_load[code.split()[1].rstrip(',')] = i
        elif op == 'ds_write_b128':
            data = code.split()[2].rstrip(',')
            if data in last_load:
                staged.append(last_load.pop(data))
        elif op == 's_barrier' and until_first_barrier:
            break
    return sorted(staged)


def _full_waits_inside_groups(body, loads, n):
    """The loads in program order, in groups of n: full waits between the first and the last load of each group."""
    assert len(loads) >= n and len(loads) % n == 0, loads
    out = []
    for g in range(0, len(loads), n):
        span = body[loads[g]:loads[g + n - 1]]
        out.append(sum(1 for c in span if c.startswith('s_waitcnt') and 'vmcnt(0)' in c))
    return out


@pytest.mark.parametrize('name', [POST_STREAM, POST_SPLIT])
def test_the_b_tile_loads_of_chunk_post_are_in_flight_together(bodies, name):
    body = bodies[name]
    loads = _staged_loads(body, until_first_barrier=True)
    assert _full_waits_inside_groups(body, loads, NST) == [0] * (len(loads) // NST), loads


@pytest.mark.parametrize('name', [LOGLIK_LAT_STREAM, LOGLIK_SPLIT])
def test_the_alpha_loads_of_a_staging_round_are_in_flight_together(bodies, name):
    body = bodies[name]
    loads = _staged_loads(body, until_first_barrier=False)
    assert _full_waits_inside_groups(body, loads, ALPHA_ROUND) == [0] * (len(loads) // ALPHA_ROUND), loads


def _descriptors(hipbuild):
    """{kernel: {vgpr_count, private_segment_fixed_size, group_segment_fixed_size}} from the notes of the code object."""
    readelf = os.path.join(os.path.dirname(hipbuild.OBJDUMP), 'llvm-readelf')
    assert os.path.exists(readelf), f'{readelf}: llvm-readelf is expected beside llvm-objdump'
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, 'lib.so')
        shutil.copy(hipbuild.LIB, copy)
        subprocess.run([hipbuild.OBJDUMP, '--offloading', copy], cwd=tmp, check=True, capture_output=True)
        obj = [f for f in os.listdir(tmp) if 'gfx950' in f][0]
        notes = subprocess.run([readelf, '--notes', os.path.join(tmp, obj)], check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r'\s+(?:- )?\.(\w+):\s+(\S+)', line)
        if not m:
            continue
        key, val = m.groups()
        if key in ('vgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size'):
            cur[key] = int(val)
        elif key == 'name' and val.startswith('_Z'):
            cur = out.setdefault(val, {})
    return out


def test_the_staged_instances_keep_their_occupancy_and_use_no_scratch():
    """Waves per SIMD by registers (512 per SIMD, allocated in eights) and workgroups per CU by LDS (160 KB): four for the
    two chunk_post instances and the LAT chunk_loglik, six for the other split chunk_loglik."""
    desc = _descriptors(_build())
    for name, want in ((POST_STREAM, 4), (POST_SPLIT, 4), (LOGLIK_LAT_STREAM, 4), (LOGLIK_SPLIT, 6)):
        d = desc[name]
        assert d['private_segment_fixed_size'] == 0, (name, d)
        by_regs = min(8, 512 // (8 * ((d['vgpr_count'] + 7) // 8)))
        by_lds = (160 * 1024) // d['group_segment_fixed_size']
        assert min(by_regs, by_lds) == want, (name, d, by_regs, by_lds)


SAMPLE = """
lib.so:	file format elf64-amdgpu

Disassembly of section .text:

0000000000001000 <_Z8kernel_av>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001000: C0060002 00000000
	s_waitcnt lgkmcnt(0)                                       // 000000001008: BF8CC07F
	global_load_dwordx4 v[2:5], v1, s[0:1]                     // 00000000100C: DC5C0000 02000001
	s_waitcnt vmcnt(0)                                         // 000000001014: BF8C0F70
	ds_write_b128 v6, v[2:5]                                   // 000000001018: D9BE0000 00000206
	global_load_dwordx4 v[2:5], v1, s[0:1] offset:4096         // 000000001020: DC5C1000 02000001
	s_waitcnt vmcnt(0)                                         // 000000001028: BF8C0F70
	ds_write_b128 v6, v[2:5] offset:4096                       // 00000000102C: D9BE1000 00000206
	s_waitcnt lgkmcnt(0)                                       // 000000001034: BF8CC07F
	s_barrier                                                  // 000000001038: BF8A0000
	s_endpgm                                                   // 00000000103C: BF810000

0000000000002000 <_Z8kernel_bv>:
	global_load_dwordx4 v[2:5], v1, s[0:1]                     // 000000002000: DC5C0000 02000001
	global_load_dwordx4 v[8:11], v1, s[0:1] offset:4096 nt     // 000000002008: DC5E1000 08000001
	buffer_load_dword v12, v1, s[8:11], 0 offen                // 000000002010: E0501000 80020C01
	s_waitcnt vmcnt(2)                                         // 000000002018: BF8C0F72
	ds_write_b128 v6, v[2:5]                                   // 00000000201C: D9BE0000 00000206
	s_waitcnt vmcnt(1) lgkmcnt(0)                              // 000000002024: BF8C0071
	ds_write_b128 v6, v[8:11] offset:4096                      // 000000002028: D9BE1000 00000806
	global_store_dword v1, v12, s[0:1]                         // 000000002030: DC700000 00000C01
	s_endpgm                                                   // 000000002038: BF810000
"""


def test_loads_in_flight_parses_a_listing():
    import loads_in_flight as lif
    ks = dict(lif.kernels(SAMPLE))
    assert list(ks) == ['_Z8kernel_av', '_Z8kernel_bv']
    a, b = lif.events(ks['_Z8kernel_av']), lif.events(ks['_Z8kernel_bv'])
    # (scalar loads, lgkmcnt-only waits and stores are not events)
    assert a == [('L', 'global_load_dwordx4'), ('W', 0), ('L', 'global_load_dwordx4'), ('W', 0), ('B', None)]
    assert b == [('L', 'global_load_dwordx4'), ('L', 'global_load_dwordx4'), ('L', 'buffer_load_dword'), ('W', 2), ('W', 1)]
    sa, sb = lif.summarize(a), lif.summarize(b)
    assert sa == {'loads': 2, 'waits': 2, 'full_waits': 2, 'max_loads_between_waits': 1, 'lone_loads_between_full_waits': 1}
    assert sb == {'loads': 3, 'waits': 2, 'full_waits': 0, 'max_loads_between_waits': 3, 'lone_loads_between_full_waits': 0}
    assert lif.compact(a) == 'L x 1 W(0) L x 1 W(0) |' and lif.compact(b) == 'L x 3 W(2) W(1)'
    # the serialised kernel is the one the staged-load check of this file rejects, the other one passes it
    assert _full_waits_inside_groups(ks['_Z8kernel_av'], _staged_loads(ks['_Z8kernel_av'], True), 2) == [1]
    assert _full_waits_inside_groups(ks['_Z8kernel_bv'], _staged_loads(ks['_Z8kernel_bv'], True), 2) == [0]
    text = lif.report(SAMPLE, ['kernel_b'])
    assert 'kernel_b' in text and 'kernel_a' not in text and 'most loads between two waits 3' in text
