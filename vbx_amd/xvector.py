"""The x-vector network of the recipes -- models/resnet.py:ResNet101 with a predict.py checkpoint -- on the GPU.

    load_checkpoint         torch.load(path)['state_dict'] (predict.py's ``--weights`` format), every tensor the network
                            needs checked by name and shape
    synthetic_state_dict    a seeded, well-scaled checkpoint (numpy only): tests, golden data, benchmarks
    blocks, walk            the block structure, written once; every convolution with the size of its input at T frames
    fold                    BatchNorm folded into each convolution in f64, packed in the order libvbx_hip.so reads
    forward_reference       the network in f64 on the CPU from the raw checkpoint (torch.nn.functional): the referee
    forward_folded          the same from the folded, packed parameters (checks fold; run_folded: on any torch device)
    ResNet101               the device path (vbx_resnet.hpp): windows [B][64][T] -> embeddings [B][E] f32; gemm='split'
                            runs layer1 .. layer4 on the f16 matrix cores with error-compensated operands; embed_ragged:
                            windows of mixed lengths in one run, bit for bit what each gives alone
    ragged_layout           where every window of a ragged batch sits at the network's four spatial levels
    split_terms             the representation of the split mode (x 2^e = hi + lo in f16), its one definition
    pack_split_weights      the split weights in the device's fragment order (unpack_split_weights: back)
    forward_split_emulated  the split mode's arithmetic on the CPU (torch, f32 accumulation)

The network: conv 3x3 1 -> 32 + BN + ReLU; Bottleneck stages of [3, 4, 23, 3] blocks, planes 32 / 64 / 128 / 256
(expansion 4), strides 1 / 2 / 2 / 2, a 1x1 conv + BN shortcut in the first block of every stage; mean and standard
deviation over time of layer4's [B][1024][8][W4]; Linear(16384 -> E).  BN in eval mode, eps 1e-5.
"""
from __future__ import annotations

import numpy as np

from . import _capi

FEAT_DIM, M_CHANNELS = 64, 32
BLOCKS, PLANES, STRIDES = (3, 4, 23, 3), (32, 64, 128, 256), (1, 2, 2, 2)
EXPANSION, BN_EPS = 4, 1e-5
H4, C4 = FEAT_DIM // 8, PLANES[-1] * EXPANSION        # layer4's rows and channels
POOL_DIM = 2 * H4 * C4                                # 16384
BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')


def _out(n, stride):
    return (n - 1) // stride + 1


def blocks():
    """The 33 Bottleneck blocks in network order: (key prefix, Cin, planes, stride, first of its stage).  The stride sits on
    conv2; the first block of a stage also has the shortcut convolution (stride 2, or 32 != 128 in layer1)."""
    cin = M_CHANNELS
    for L, (n, planes, stride) in enumerate(zip(BLOCKS, PLANES, STRIDES), 1):
        for i in range(n):
            yield f'layer{L}.{i}.', cin, planes, stride if i == 0 else 1, i == 0
            cin = EXPANSION * planes


def conv_specs():
    """Every convolution in the order the device reads them: (conv key, BN key, kernel size, stride, Cin, Cout)."""
    out = [('conv1', 'bn1', 3, 1, 1, M_CHANNELS)]
    for p, cin, planes, s, first in blocks():
        out += [(p + 'conv1', p + 'bn1', 1, 1, cin, planes), (p + 'conv2', p + 'bn2', 3, s, planes, planes),
                (p + 'conv3', p + 'bn3', 1, 1, planes, EXPANSION * planes)]
        if first:
            out.append((p + 'shortcut.0', p + 'shortcut.1', 1, s, cin, EXPANSION * planes))
    return out


def walk(T: int):
    """(spec, H, W) of every convolution after the stem at T frames, in conv_specs() order: H x W is what it reads."""
    specs, k, H, W = conv_specs(), 1, FEAT_DIM, T
    for _, _, _, s, first in blocks():
        Ho, Wo = _out(H, s), _out(W, s)
        for hw in ((H, W), (H, W), (Ho, Wo), (H, W))[:4 if first else 3]:
            yield (specs[k],) + hw
            k += 1
        H, W = Ho, Wo


LEVELS = 4                                             # spatial levels of the network: 64, 32, 16, 8 rows


def ragged_layout(lengths):
    """The layout of a ragged batch -- windows of lengths[b] >= 1 frames, in any order -- as the device builds it
    (vbx_host_resnet.hpp: rn_batch): -> (pos int64 [4][n + 1], wid int32 [4][n]).  At level l (64 >> l rows) window b
    is wid[l][b] wide (the stride-2 output size applied l times to lengths[b]) and its [H_l][wid[l][b]][C] block starts at
    position pos[l][b] of the concatenated activation tensor; pos[l][n] = M_l, all positions of the level."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.size == 0:
        raise ValueError('ragged_layout: no windows')
    if lengths.min() <= 0:
        b = int(np.argmax(lengths <= 0))
        raise ValueError(f'ragged_layout: window {b} has {int(lengths[b])} frames, need at least 1')
    wid = np.empty((LEVELS, lengths.size), dtype=np.int64)
    wid[0] = lengths
    for l in range(1, LEVELS):
        wid[l] = _out(wid[l - 1], 2)
    pos = np.zeros((LEVELS, lengths.size + 1), dtype=np.int64)
    pos[:, 1:] = np.cumsum(wid * (FEAT_DIM >> np.arange(LEVELS))[:, None], axis=1)
    return pos, wid.astype(np.int32)


def required_shapes(embed_dim: int) -> dict:
    shapes = {}
    for conv, bn, k, _, cin, cout in conv_specs():
        shapes[conv + '.weight'] = (cout, cin, k, k)
        for key in BN_KEYS:
            shapes[f'{bn}.{key}'] = (cout,)
    shapes['embedding.weight'] = (embed_dim, POOL_DIM)
    shapes['embedding.bias'] = (embed_dim,)
    return shapes


def n_params(embed_dim: int) -> int:
    """f32 values of the folded network (vbx_resnet_create's n_params)."""
    return sum(k * k * cin * cout + cout for _, _, k, _, cin, cout in conv_specs()) + POOL_DIM * embed_dim + embed_dim


def _numpy(t):
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t)


def check_state_dict(sd, embed_dim: int | None = None) -> dict:
    """The tensors ResNet101 needs, as numpy arrays, after checking every one by name and shape.  Extra keys (such as
    ``num_batches_tracked``) are ignored; a missing or misshapen tensor is an error that names it.  (predict.py loads with
    strict=False and would run a partly random network instead.)"""
    if not isinstance(sd, dict):
        raise ValueError(f'a checkpoint state_dict must be a dict, got {type(sd).__name__}')
    if embed_dim is None:
        if 'embedding.weight' not in sd:
            raise ValueError(_missing_message(sd, ['embedding.weight']))
        embed_dim = int(np.shape(_numpy(sd['embedding.weight']))[0])
    shapes = required_shapes(int(embed_dim))
    missing = [k for k in shapes if k not in sd]
    if missing:
        raise ValueError(_missing_message(sd, missing))
    out = {}
    for k, shape in shapes.items():
        a = _numpy(sd[k])
        if tuple(a.shape) != shape:
            raise ValueError(f'checkpoint tensor {k} has shape {tuple(a.shape)}, ResNet101 (embed_dim {embed_dim}) needs {shape}')
        if not np.issubdtype(a.dtype, np.floating):
            raise ValueError(f'checkpoint tensor {k} is {a.dtype}, not floating point')
        out[k] = a
    return out


def _missing_message(sd, missing):
    msg = f'checkpoint lacks {len(missing)} tensor(s) ResNet101 needs, first {missing[0]}'
    if any(str(k).startswith('module.') for k in sd):
        msg += " (its keys start with 'module.': a DataParallel state_dict; strip the prefix)"
    return msg


def load_checkpoint(path, embed_dim: int | None = None) -> dict:
    """predict.py's ``--weights`` file: ``torch.load(path)['state_dict']``, checked (check_state_dict)."""
    import torch
    ck = torch.load(path, map_location='cpu', weights_only=True)
    if not isinstance(ck, dict) or 'state_dict' not in ck:
        raise ValueError(f"{path}: not a checkpoint of predict.py's format (a dict with a 'state_dict')")
    return check_state_dict(ck['state_dict'], embed_dim)


def synthetic_state_dict(seed: int, embed_dim: int = 256) -> dict:
    """A deterministic f32 checkpoint whose activations stay in range through all 33 blocks: conv weights N(0, 2 / fan_in);
    BN gamma U(0.2, 0.5) for bn3, U(0.8, 1.2) elsewhere; beta and running mean 0.1 N(0, 1); running variance
    U(0.5, 1.5); embedding weight N(0, 1 / 16384), bias 0.1 N(0, 1).  numpy's PCG64 only, drawn in conv_specs() order."""
    rng = np.random.default_rng(seed)
    sd = {}
    for conv, bn, k, _, cin, cout in conv_specs():
        sd[conv + '.weight'] = rng.normal(0.0, np.sqrt(2.0 / (cin * k * k)), (cout, cin, k, k))
        lo, hi = (0.2, 0.5) if bn.endswith('bn3') else (0.8, 1.2)
        sd[bn + '.weight'] = rng.uniform(lo, hi, cout)
        sd[bn + '.bias'] = 0.1 * rng.standard_normal(cout)
        sd[bn + '.running_mean'] = 0.1 * rng.standard_normal(cout)
        sd[bn + '.running_var'] = rng.uniform(0.5, 1.5, cout)
    sd['embedding.weight'] = rng.normal(0.0, np.sqrt(1.0 / POOL_DIM), (embed_dim, POOL_DIM))
    sd['embedding.bias'] = 0.1 * rng.standard_normal(embed_dim)
    return {k: v.astype(np.float32) for k, v in sd.items()}


def pool_order() -> np.ndarray:
    """perm[p] = the reference's pooled index (mean: c 8 + h, std: 8192 + c 8 + h) of the device's pooled index p
    (mean: h 1024 + c, std: 8192 + h 1024 + c)."""
    p = np.arange(H4 * C4)
    ref = (p % C4) * H4 + p // C4
    return np.concatenate([ref, H4 * C4 + ref])


def fold(sd) -> np.ndarray:
    """The folded network, f64, in the device's order (include/vbx_hip.h: vbx_resnet_create): per convolution
    W[o] gamma[o] / sqrt(var[o] + eps) laid out [(r kw + s) Cin + c][o], then bias beta - mean gamma / sqrt(var + eps);
    then the embedding [16384][E] with its rows in pooling order, and its bias."""
    sd = check_state_dict(sd)
    parts = []
    for conv, bn, k, _, cin, cout in conv_specs():
        w = sd[conv + '.weight'].astype(np.float64)
        g, b, m, v = (sd[f'{bn}.{key}'].astype(np.float64) for key in BN_KEYS)
        scale = g / np.sqrt(v + BN_EPS)
        parts.append((w * scale[:, None, None, None]).transpose(2, 3, 1, 0).reshape(-1))
        parts.append(b - m * scale)
    parts.append(sd['embedding.weight'].astype(np.float64)[:, pool_order()].T.reshape(-1))
    parts.append(sd['embedding.bias'].astype(np.float64))
    return np.concatenate(parts)


def _run_network(x, conv, embed, pool_dtype=None):
    """The network's one loop: the stem, the 33 blocks, the statistics over time, the embedding.  conv(k, h, stride, relu,
    res) applies convolution k of conv_specs() to h (+ res, then ReLU); the pooling sums in pool_dtype (None: h's own);
    embed(mean, std) [B][1024][8] each -> [B][E]."""
    import torch
    with torch.no_grad():
        h, k = conv(0, x[:, None], 1, True, None), 1
        for _, _, _, s, first in blocks():
            o = conv(k + 1, conv(k, h, 1, True, None), s, True, None)
            sc = conv(k + 3, h, s, False, None) if first else h
            h = conv(k + 2, o, 1, True, sc)                    # (conv3 comes before the shortcut in the parameter order)
            k += 4 if first else 3
        if pool_dtype is not None:
            h = h.to(pool_dtype)
        mean = h.mean(dim=-1)
        std = torch.sqrt((h * h).mean(dim=-1) - mean ** 2 + 1e-10)
        return embed(mean, std)


def forward_reference(sd, x) -> np.ndarray:
    """ResNet.forward (models/resnet.py:130-145) with BN in eval mode, in f64 on the CPU: x [B][64][T] -> [B][E]."""
    import torch
    import torch.nn.functional as F
    sd = check_state_dict(sd)
    t = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in sd.items()}
    specs = conv_specs()

    def conv(k, h, stride, relu, res):
        key, bn, ks = specs[k][:3]
        h = F.conv2d(h, t[key + '.weight'], stride=stride, padding=ks // 2)
        h = F.batch_norm(h, t[bn + '.running_mean'], t[bn + '.running_var'], t[bn + '.weight'], t[bn + '.bias'],
                         training=False, eps=BN_EPS)
        if res is not None:
            h = h + res
        return F.relu(h) if relu else h

    def embed(mean, std):
        return torch.cat([mean.flatten(1), std.flatten(1)], 1) @ t['embedding.weight'].T + t['embedding.bias']

    return _run_network(torch.from_numpy(np.asarray(x, dtype=np.float64)), conv, embed).numpy()


def folded_tensors(params, embed_dim: int, device='cpu', dtype=None) -> list:
    """fold()'s packed parameters as torch tensors in conv2d's layout: [(weight [Cout][Cin][k][k], bias)] in
    conv_specs() order, then (embedding [16384][E], bias)."""
    import torch
    dtype = dtype or torch.float64
    params = torch.from_numpy(np.asarray(params, dtype=np.float64))
    assert params.numel() == n_params(embed_dim)
    out, off = [], 0
    for _, _, k, _, cin, cout in conv_specs():
        w = params[off:off + k * k * cin * cout].reshape(k, k, cin, cout).permute(3, 2, 0, 1)
        off += k * k * cin * cout
        out.append((w, params[off:off + cout]))
        off += cout
    out.append((params[off:off + POOL_DIM * embed_dim].reshape(POOL_DIM, embed_dim), params[off + POOL_DIM * embed_dim:]))
    return [(w.to(device=device, dtype=dtype).contiguous(), b.to(device=device, dtype=dtype)) for w, b in out]


def _embed_folded(tensors):
    """embed() of _run_network for folded_tensors(): the pooled vector in the device's order (h 1024 + c)."""
    import torch
    ew, eb = tensors[-1]
    return lambda mean, std: torch.cat([mean.transpose(1, 2).flatten(1), std.transpose(1, 2).flatten(1)], 1).to(ew.dtype) @ ew + eb


def run_folded(tensors, x):
    """The network on folded_tensors(): x [B][64][T] tensor of their device and dtype -> [B][E]."""
    import torch.nn.functional as F

    def conv(k, h, stride, relu, res):
        w, b = tensors[k]
        h = F.conv2d(h, w, b, stride=stride, padding=w.shape[-1] // 2)
        if res is not None:
            h = h + res
        return F.relu(h) if relu else h

    return _run_network(x, conv, _embed_folded(tensors))


def forward_folded(params, embed_dim: int, x) -> np.ndarray:
    """The network from fold()'s packed parameters, in f64 on the CPU (what the device computes, in f64)."""
    import torch
    return run_folded(folded_tensors(params, embed_dim), torch.from_numpy(np.asarray(x, dtype=np.float64))).numpy()


SPLIT_TOP = 14                                         # a scaling group's largest magnitude sits in [2^13, 2^14)


def split_exponent(amax) -> np.ndarray:
    """e with amax 2^e in [2^13, 2^14) (clamped to +-100); 0 where amax is zero or not finite."""
    amax = np.asarray(amax, dtype=np.float32)
    ok = np.isfinite(amax) & (amax > 0)
    _, ex = np.frexp(np.where(ok, amax, np.float32(1.0)))
    return np.where(ok, np.clip(SPLIT_TOP - ex, -100, 100), 0).astype(np.int32)


def split_terms(x, amax):
    """The split mode's representation of f32 values x under the scale of their group's largest magnitude amax (an array
    that broadcasts against x): -> (hi, lo, e) with x 2^e = hi + lo up to 2^-23 |x|, hi = f16(x 2^e), lo = f16(x 2^e - hi)
    (both float16, round to nearest even), e = split_exponent(amax).  What the device computes, operation for operation."""
    x = np.asarray(x, dtype=np.float32)
    e = split_exponent(amax)
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.ldexp(x, e).astype(np.float32)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo, e


def _finite_amax(a, axis):
    a = np.abs(np.asarray(a, dtype=np.float32))
    return np.where(np.isfinite(a), a, np.float32(0)).max(axis=axis)


def pack_split_weights(w):
    """w [K][Cout] f32 (K a multiple of 16, Cout of 32) -> (frag float16 [K / 16][Cout / 32][hi | lo][64][8], e int32 [Cout]):
    one scale per output channel, in the fragment order of the B operand of v_mfma_f32_32x32x16_f16 -- lane l holds
    B[k = 8 (l >> 5) + j][column l & 31] in element j.  What vbx_resnet_create stores (vbx_resnet_split_weights)."""
    w = np.asarray(w, dtype=np.float32)
    K, Cout = w.shape
    assert K % 16 == 0 and Cout % 32 == 0
    aw = np.abs(w)
    amax = np.fmax.reduce(aw, axis=0) if K else np.zeros(Cout, np.float32)          # (a NaN does not count)
    hi, lo, e = split_terms(w, amax[None, :])
    t = np.stack([hi, lo])                                                           # [term][k][n]
    # k = 16 kstep + 8 h + j, n = 32 cb + r  ->  [kstep][cb][term][lane = 32 h + r][j]
    frag = t.reshape(2, K // 16, 2, 8, Cout // 32, 32).transpose(1, 4, 0, 2, 5, 3).reshape(K // 16, Cout // 32, 2, 64, 8)
    return np.ascontiguousarray(frag), e.reshape(-1)


def unpack_split_weights(frag, e):
    """pack_split_weights backwards: -> (hi, lo) float16 [K][Cout]."""
    ksteps, cbs = frag.shape[:2]
    t = frag.reshape(ksteps, cbs, 2, 2, 32, 8).transpose(2, 0, 3, 5, 1, 4).reshape(2, ksteps * 16, cbs * 32)
    assert t.shape[2] == len(e)
    return t[0], t[1]


def forward_split_emulated(params, embed_dim: int, x) -> np.ndarray:
    """The split mode on the CPU (torch): the stem, the pooling (f64 sums) and the embedding as the exact mode has them in
    f32; every other convolution as lo hi + hi lo + hi hi of split_terms' operands -- activations scaled per window (the
    largest finite magnitude), weights per output channel -- accumulated in f32, then 2^-(e_window + e_channel), + bias,
    + res, ReLU.  torch sums in another order than the device, so this shows the mode's accuracy, not its bits."""
    import torch
    import torch.nn.functional as F
    tens = folded_tensors(np.asarray(params, dtype=np.float32), embed_dim, dtype=torch.float32)

    def conv(k, h, stride, relu, res):
        w, b = tens[k]
        cout, cin, ks, _ = w.shape
        if k == 0:                                                             # the stem stays exact
            return F.relu(F.conv2d(h, w, b, padding=1))
        wk = w.permute(2, 3, 1, 0).reshape(ks * ks * cin, cout).numpy()
        whi, wlo, we = split_terms(wk, np.fmax.reduce(np.abs(wk), axis=0)[None, :])
        hn = h.numpy()
        ahi, alo, ae = split_terms(hn, _finite_amax(hn.reshape(len(hn), -1), 1)[:, None, None, None])
        back = lambda a: torch.from_numpy(a.astype(np.float32).reshape(ks, ks, cin, cout)).permute(3, 2, 0, 1).contiguous()
        t = lambda a: torch.from_numpy(a.astype(np.float32))
        kw = dict(stride=stride, padding=ks // 2)
        acc = F.conv2d(t(alo), back(whi), **kw) + F.conv2d(t(ahi), back(wlo), **kw) + F.conv2d(t(ahi), back(whi), **kw)
        scale = np.ldexp(np.float32(1), -(ae.reshape(-1, 1, 1, 1) + we.reshape(1, -1, 1, 1))).astype(np.float32)
        y = acc * torch.from_numpy(scale) + b.reshape(1, -1, 1, 1)
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y

    x = torch.from_numpy(np.asarray(x, dtype=np.float32))
    return _run_network(x, conv, _embed_folded(tens), pool_dtype=torch.float64).numpy()


class ResNet101:
    """The network on one device.  ``embed(x)``: x [B][64][T] f32 (numpy, or a torch tensor on the device) -> [B][E] f32
    of the same kind.  gemm: 'exact' (default: the f32 matrix instructions) or 'split' (f16 matrix instructions on
    error-compensated operand pairs: f32-level accuracy, faster, other bits).  Runs on the device context's stream, the front end's (vbx_amd.fbank), so that ``embed_windows``
    goes from features to embeddings without a host round trip or a torch allocation."""

    def __init__(self, sd, device: int = 0, gemm: str = 'exact'):
        if gemm not in ('exact', 'split'):
            raise ValueError(f"gemm must be 'exact' or 'split', got {gemm!r}")
        sd = check_state_dict(sd)
        self.embed_dim = int(sd['embedding.weight'].shape[0])
        self.device = int(device)
        if _capi._lib is None:
            try:                                      # (PyTorch's HIP runtime first: see fbank.FrontEnd)
                import torch  # noqa: F401
            except ImportError:
                pass
        self.ctx = _capi.default_context(self.device)
        self.dev = _capi.ResNetDevice(self.ctx, fold(sd).astype(np.float32), self.embed_dim, gemm=gemm)

    def gemm_in_effect(self) -> str:
        """'exact' or 'split': how the convolutions of the last embed() multiplied."""
        return self.dev.gemm_in_effect()

    @classmethod
    def from_checkpoint(cls, src, device: int = 0, embed_dim: int | None = None, gemm: str = 'exact') -> 'ResNet101':
        """src: a checkpoint path (predict.py's ``--weights``) or a state_dict."""
        sd = load_checkpoint(src, embed_dim) if isinstance(src, (str, bytes)) or hasattr(src, '__fspath__') else \
            check_state_dict(src, embed_dim)
        return cls(sd, device, gemm)

    def embed(self, x):
        if hasattr(x, 'data_ptr'):
            import torch
            if x.dim() != 3 or x.shape[1] != FEAT_DIM or x.dtype != torch.float32 or not x.is_cuda:
                raise ValueError(f'embed: expected a float32 [B][{FEAT_DIM}][T] tensor on the GPU')
            x = x.contiguous()
            B, _, T = x.shape
            out = torch.empty((B, self.embed_dim), dtype=torch.float32, device=x.device)
            torch.cuda.current_stream(x.device).synchronize()      # x written, out's block free, on torch's stream
            if B:
                self.dev.run(B, T, x_ptr=x.data_ptr(), out_ptr=out.data_ptr())
            return out
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 3 or x.shape[1] != FEAT_DIM:
            raise ValueError(f'embed: expected [B][{FEAT_DIM}][T], got {x.shape}')
        if x.shape[0] == 0:
            return np.empty((0, self.embed_dim), dtype=np.float32)
        return self.dev.run(x.shape[0], x.shape[2], x)

    def embed_windows(self, fe, starts, length: int, out_ptr=None) -> np.ndarray:
        """Embeddings of the windows ``fe.windows(starts, length)`` of a front end on the same device: gathered straight
        into the network's input buffer.  With ``out_ptr`` (a device address with room for [len(starts)][E] f32) they stay
        on the device and None is returned."""
        starts = np.asarray(starts, dtype=np.int64)
        ptr = self.dev.input_buffer(len(starts), length)
        fe.dev.windows(starts, length, dst_ptr=ptr)
        return self.dev.run(len(starts), length, x_ptr=ptr, out_ptr=out_ptr)

    def embed_ragged(self, windows, lengths=None):
        """Embeddings [n][E] of windows of mixed lengths in one run of the network; every one has the bits ``embed`` gives
        that window alone.  windows: a list of [64][T_b] f32 arrays; or, with ``lengths`` [n], their blocks end to end as one
        flat array of 64 sum(lengths) values -- numpy, or a torch tensor on the device (then the result is one too)."""
        if lengths is None:
            windows = [np.ascontiguousarray(w, dtype=np.float32) for w in windows]
            for b, w in enumerate(windows):
                if w.ndim != 2 or w.shape[0] != FEAT_DIM:
                    raise ValueError(f'embed_ragged: window {b}: expected [{FEAT_DIM}][T], got {w.shape}')
            lengths = [w.shape[1] for w in windows]
            windows = np.concatenate([w.reshape(-1) for w in windows]) if windows else np.empty(0, np.float32)
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if lengths.size == 0:
            return np.empty((0, self.embed_dim), dtype=np.float32)
        if lengths.min() <= 0:
            b = int(np.argmax(lengths <= 0))
            raise ValueError(f'embed_ragged: window {b} has {int(lengths[b])} frames, need at least 1')
        total = FEAT_DIM * int(lengths.sum())
        if hasattr(windows, 'data_ptr'):
            import torch
            if windows.dtype != torch.float32 or not windows.is_cuda or windows.numel() != total:
                raise ValueError(f'embed_ragged: expected a float32 tensor of {total} values on the GPU')
            x = windows.contiguous()
            out = torch.empty((lengths.size, self.embed_dim), dtype=torch.float32, device=x.device)
            torch.cuda.current_stream(x.device).synchronize()      # x written, out's block free, on torch's stream
            self.dev.run_ragged(lengths, x_ptr=x.data_ptr(), out_ptr=out.data_ptr())
            return out
        x = np.ascontiguousarray(windows, dtype=np.float32).reshape(-1)
        if x.size != total:
            raise ValueError(f'embed_ragged: {x.size} values given, the lengths ask for {FEAT_DIM} x {int(lengths.sum())}')
        return self.dev.run_ragged(lengths, x)

    def embed_windows_ragged(self, fe, starts, lengths, out_ptr=None) -> np.ndarray:
        """Embeddings of the windows of lengths[w] frames from feature rows starts[w] of a front end on the same device:
        one gather into the network's input buffer, one run of the network.  With ``out_ptr`` (a device address with room
        for [len(starts)][E] f32) they stay on the device and None is returned."""
        starts = np.asarray(starts, dtype=np.int64).reshape(-1)
        lengths = np.asarray(lengths, dtype=np.int32).reshape(-1)
        if starts.size != lengths.size:
            raise ValueError(f'embed_windows_ragged: {starts.size} starts, {lengths.size} lengths')
        if starts.size == 0:
            return None if out_ptr is not None else np.empty((0, self.embed_dim), dtype=np.float32)
        ptr = self.dev.input_buffer_ragged(lengths)
        fe.dev.windows_ragged(starts, lengths, dst_ptr=ptr)
        return self.dev.run_ragged(lengths, x_ptr=ptr, out_ptr=out_ptr)

    def times(self) -> dict:
        """Device ms of the last run: stem, layer1 .. layer4, pool_embed."""
        return self.dev.times()


def flops(T: int) -> dict:
    """Multiply-add FLOPs (2 per MAC) of one window of T frames, per stage."""
    out = {'stem': 2 * 9 * M_CHANNELS * FEAT_DIM * T}
    for (key, _, ks, s, cin, cout), H, W in walk(T):
        stage = key.partition('.')[0]                      # 'layer1' .. 'layer4'
        out[stage] = out.get(stage, 0) + 2 * _out(H, s) * _out(W, s) * ks * ks * cin * cout
    return out
