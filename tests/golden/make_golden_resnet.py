#!/usr/bin/env python
"""The x-vector network -- the reference's own models/resnet.py:ResNet101 with a synthetic checkpoint -- captured while the
UNCHANGED /root/reference/VBx/predict.py runs over the five recordings of fbank_cases.npz (authoring container only).

It reuses make_golden_fbank.py's shims, except that ``models.resnet`` is the reference's module itself, with hooks on
ResNet101 that note every network input and output.  predict.py runs on the CPU with ``--gpus '' --model ResNet101
--weights <vbx_amd.xvector.synthetic_state_dict(SEED) saved as {'state_dict': ...}>``.  Every recorded input is asserted to
be its window of fbank_cases.npz's features, so the GPU tests take their inputs from that file.

    tests/golden/resnet_cases.npz
        seed, embed_dim                      the checkpoint: synthetic_state_dict(seed, embed_dim)
        win_rec, win_seg, win_start, win_len the window plan: recording (index into fbank_cases' names), processed segment,
                                             first frame within it, frames
        emb_ref   f32 [41][E]                the reference's embeddings, in predict.py's order
        emb_f64   f64 [41][E]                the referee: vbx_amd.xvector.forward_reference (own f64 functional forward)
        ark uint8, segments str              the two output files, byte for byte
"""
import os
import runpy
import sys
import tempfile
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path[:0] = [REPO, HERE]

from make_golden_fbank import SHIMS as FBANK_SHIMS     # noqa: E402
from vbx_amd import xvector                            # noqa: E402
from vbx_amd.fbank import write_wav                    # noqa: E402

SEED, EMBED_DIM = 20261016, 256

SHIMS = dict(FBANK_SHIMS)
SHIMS['models/resnet.py'] = '''
    import importlib.util
    _spec = importlib.util.spec_from_file_location('_ref_resnet', '%(ref)s/VBx/models/resnet.py')
    _ref = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(_ref)
    globals().update({k: v for k, v in vars(_ref).items() if not k.startswith('__')})
    INPUTS, OUTPUTS = [], []
    def ResNet101(*a, **kw):
        m = _ref.ResNet101(*a, **kw)
        # (before forward: it unsqueezes its input in place)
        m.register_forward_pre_hook(lambda mod, inp: INPUTS.append(inp[0].detach().cpu().numpy().copy()))
        m.register_forward_hook(lambda mod, inp, out: OUTPUTS.append(out.detach().cpu().numpy().copy()))
        return m
''' % {'ref': REF}


def main():
    G = np.load(os.path.join(HERE, 'fbank_cases.npz'))
    names = [str(n) for n in G['names']]
    rates = [int(r) for r in G['rates']]
    sd = xvector.synthetic_state_dict(SEED, EMBED_DIM)
    out = {'seed': np.int64(SEED), 'embed_dim': np.int64(EMBED_DIM)}
    with tempfile.TemporaryDirectory() as tmp:
        wav, lab = os.path.join(tmp, 'wav'), os.path.join(tmp, 'lab')
        os.makedirs(wav)
        os.makedirs(lab)
        for name, sr in zip(names, rates):
            write_wav(os.path.join(wav, name + '.wav'), G['sig_' + name], sr)
            with open(os.path.join(lab, name + '.lab'), 'w') as f:
                f.write(str(G['lab_' + name]))
        with open(os.path.join(tmp, 'list.txt'), 'w') as f:
            f.write(''.join(n + '\n' for n in names))
        torch.save({'state_dict': {k: torch.from_numpy(v) for k, v in sd.items()}}, os.path.join(tmp, 'w.pth'))
        shims = os.path.join(tmp, 'shims')
        for rel, src in SHIMS.items():
            os.makedirs(os.path.dirname(os.path.join(shims, rel)), exist_ok=True)
            with open(os.path.join(shims, rel), 'w') as f:
                f.write(textwrap.dedent(src))
        ark, seg = os.path.join(tmp, 'out.ark'), os.path.join(tmp, 'out.seg')
        argv = ['--gpus', '', '--model', 'ResNet101', '--weights', os.path.join(tmp, 'w.pth'), '--in-file-list',
                os.path.join(tmp, 'list.txt'), '--in-lab-dir', lab, '--in-wav-dir', wav, '--out-ark-fn', ark, '--out-seg-fn', seg]
        script = f'{REF}/VBx/predict.py'
        old_argv, old_path = sys.argv, list(sys.path)
        sys.argv = [script] + argv
        sys.path[:0] = [shims, f'{REF}/VBx']
        for name in ('features', 'kaldi_io', 'soundfile', 'onnxruntime', 'models', 'models.resnet'):
            sys.modules.pop(name, None)
        try:
            runpy.run_path(script, run_name='__main__')
            mod = sys.modules['models.resnet']
            inputs, outputs = mod.INPUTS, mod.OUTPUTS
        finally:
            sys.argv, sys.path[:] = old_argv, old_path
        with open(ark, 'rb') as f:
            out['ark'] = np.frombuffer(f.read(), dtype=np.uint8)
        with open(seg) as f:
            out['segments'] = np.array(f.read())
    # the windows in predict.py's order (predict.py:179-200); each input must be its window of the fixture's features
    plan, wi = [], 0
    for r, name in enumerate(names):
        rows = G['rows_' + name]
        off = np.concatenate([[0], np.cumsum(rows)])
        for s in range(len(rows)):
            f = G['fea_' + name][off[s]:off[s + 1]]
            slen, start = len(f), -24
            for start in range(0, slen - 144, 24):
                plan.append((r, s, start, 144))
            if slen - start - 24 >= 10:
                plan.append((r, s, start + 24, slen - start - 24))
    assert len(plan) == len(inputs) == len(outputs), (len(plan), len(inputs), len(outputs))
    for (r, s, a, n), x in zip(plan, inputs):
        rows = G['rows_' + names[r]]
        f = G['fea_' + names[r]][int(np.sum(rows[:s])):int(np.sum(rows[:s + 1]))]
        assert x.shape == (1, 64, n) and np.array_equal(x[0].T, f[a:a + n])
        wi += 1
    plan = np.array(plan, dtype=np.int64)
    out['win_rec'], out['win_seg'], out['win_start'], out['win_len'] = plan.T
    out['emb_ref'] = np.concatenate(outputs).astype(np.float32)
    out['emb_f64'] = np.concatenate([xvector.forward_reference(sd, x) for x in inputs])
    err = np.abs(out['emb_ref'] - out['emb_f64']).max(1) / np.abs(out['emb_f64']).max(1)
    path = os.path.join(HERE, 'resnet_cases.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', wi, 'windows; lengths', sorted(set(plan[:, 3].tolist())),
          f'; reference f32 vs f64: max {err.max():.2e} of max|e|')


if __name__ == '__main__':
    main()
