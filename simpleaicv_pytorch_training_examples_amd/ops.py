"""torch.autograd.Functions over the C-ABI of libsaicv_hip.so.

Activations are NCHW-shaped, NHWC-strided (torch.channels_last) tensors in the compute dtype
(bf16 under autocast = perf mode, fp32 otherwise = parity mode).  Statistics, logits, losses
and every parameter gradient are fp32, as under the reference's autocast region
(reference tools/scripts.py:153-156).
"""
import collections
import ctypes
import weakref

import torch

from . import _lib
from ._lib import ConvDesc, check, dtype_code, lib, ptr, require_gpu, stream

_weights_epoch = [0]


class KernelTimer:
    """HIP-event bracketing of selected launches on torch's current stream (the stream every
    saicv kernel is launched on).  bench.py enables it to price the dominant kernel against
    its roofline from live measurements; it is off by default (zero overhead)."""
    enabled = False
    only = None           # optional set of tags to bracket (every event pair costs host time: ~1400 per ResNet-50 step
                          # with all tags made the bench host-bound and 7 % slower; bench.py brackets the dominant kernel)
    records = []          # (tag, start_event, end_event, algorithmic_flops, algorithmic_bytes)
    PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12      # dense bf16 MFMA, HBM3E (MI355X_MICROARCH.md)

    @classmethod
    def begin(cls, tag=None):
        if not cls.enabled or (cls.only is not None and tag not in cls.only):
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    @classmethod
    def end(cls, e0, tag, flops, nbytes):
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        cls.records.append((tag, e0, e1, flops, nbytes))

    @classmethod
    def summary(cls):
        """{tag: dict(calls, ms, flops, bytes, bound_ms)}; call after torch.cuda.synchronize().
        bound_ms = sum over the launches of max(flops / MFMA peak, bytes / HBM peak): what the SHAPES allow."""
        out = {}
        for tag, e0, e1, fl, by in cls.records:
            d = out.setdefault(tag, {'calls': 0, 'ms': 0.0, 'flops': 0.0, 'bytes': 0.0, 'bound_ms': 0.0})
            d['calls'] += 1
            d['ms'] += e0.elapsed_time(e1)
            d['flops'] += fl
            d['bytes'] += by
            d['bound_ms'] += max(fl / cls.PEAK_FLOPS, by / cls.PEAK_BYTES) * 1e3
        return out


def bump_weights_epoch():
    """Called by the flat-arena optimizer after it rewrote parameters through raw pointers: the step boundary."""
    _weights_epoch[0] += 1
    _ZeroPool.reset()


class _ZeroPool:
    """fp32 scratch that is all zeros when handed out: the few-row buffers BatchNorm statistics are added into with atomics
    (ConvBnActFn, SAICV_BN_INLINE).  One memset per step boundary instead of one per layer; the slices keep their addresses
    from step to step, so a captured step replays against the same memory."""
    CHUNK = 1 << 20            # floats
    LIMIT = 64 << 20           # floats handed out without a step boundary before falling back to torch.zeros per request
    chunks = []                # [tensor, used]
    handed = 0

    @classmethod
    def take(cls, want, device):
        n = (want + 63) // 64 * 64                 # slices start on 256-byte boundaries
        if cls.handed > cls.LIMIT:                 # nobody calls the step boundary (a foreign optimizer): stay bounded
            return torch.zeros(want, dtype=torch.float32, device=device)
        cls.handed += n
        for ch in cls.chunks:
            if ch[0].device == device and ch[1] + n <= ch[0].numel():
                v = ch[0][ch[1]:ch[1] + want]
                ch[1] += n
                return v
        t = torch.zeros(max(n, cls.CHUNK), dtype=torch.float32, device=device)
        cls.chunks.append([t, n])
        return t[:want]

    @classmethod
    def zero_all(cls):
        """Zeroes every chunk in full (a few MB).  A captured step replays its BatchNorm atomics into fixed slices and
        needs them zero whatever ran eagerly since the last step boundary (a train-mode forward without an optimizer step
        takes the same slices and leaves its sums behind): engine.StepGraph captures this call in front of the step."""
        for ch in cls.chunks:
            ch[0].zero_()

    @classmethod
    def reset(cls):
        for ch in cls.chunks:
            if ch[1]:
                ch[0][:ch[1]].zero_()
                ch[1] = 0
        cls.handed = 0


def _stat_rows(tile_rows):
    """Rows the atomically accumulated statistics are spread over: enough to keep the atomics of a many-tile layer apart,
    few enough for every workgroup of the consuming kernel to sum them.  Each row is a chain of fp32 additions whose rounding the
    variance of an off-centre channel amplifies by (mean / std)^2; the error goes as sqrt(tile rows) / rows, so the longest chains -- the
    128-row tiles of the 56 x 56 layers at batch 256, 6272 tile rows -- take 32 rows."""
    return 32 if tile_rows >= 4096 else 8 if tile_rows >= 512 else 4 if tile_rows >= 64 else 2 if tile_rows >= 8 else 1


def _arena_grad(t):
    """t.grad when it is a persistent view into the engine's flat gradient arena that kernels
    may accumulate into directly (set up by engine.FlatArena), else None.

    A kernel that wrote in place returns None for that input; autograd still runs the leaf's
    AccumulateGrad node -- exactly once per backward, after EVERY use of the parameter has run its
    backward -- and with it the post-accumulate hook engine.FlatArena registers.  That hook is the
    only "gradient complete" signal the DDP engine and the optimizers act on, so a parameter used
    several times per step (DETR's shared decoder norm, the SAM decoder passes) is never reduced
    or counted early."""
    if t is None or not getattr(t, '_saicv_direct', False):
        return None
    g = t.grad
    if g is None or g.dtype != torch.float32 or g.stride() != t.stride():
        return None
    return g


import os as _os

# (Weight gradients on a second HIP stream were tried twice and measured neutral to -2 %: profiles/r05_nt_experiments.md.)
# BatchNorm-backward traffic cuts in residual networks: the shortcut gradient travels as
# (dz, ReLU-mask) instead of a masked copy, and a BatchNorm's backward reduction comes out of the epilogue of the data
# gradient that produces its dz.  SAICV_BN_FUSE=0 restores the three-pass form (A/B runs, tests of both paths).
BN_FUSE = _os.environ.get('SAICV_BN_FUSE', '1') == '1'
# BatchNorm statistics added atomically into a few zeroed rows and finalised inside the consuming kernel (no partial-reduce /
# finalize launches); SAICV_BN_INLINE=0 keeps one partial row per tile row and the finalize kernels (bit-reproducible sums)
BN_INLINE = _os.environ.get('SAICV_BN_INLINE', '1') == '1'


def set_deterministic(on=True):
    """The engine's counterpart of `torch.backends.cudnn.deterministic = True` (reference tools/utils.py:106-107): with `on`, every
    reduction of libsaicv_hip.so is ordered (csrc/det.h: partials parked side by side, folded in index order) and the BatchNorm
    statistics of the convolution epilogues take the fixed-order partial rows -- an fp32 step is then bit-reproducible run to run.
    Costs a fold launch per weight gradient; the fast default adds partials with fp32 atomics in completion order.
    tools.utils.set_seed() turns it on (SAICV_DETERMINISTIC=0 in the environment keeps the fast path, as bench.py does);
    SAICV_DETERMINISTIC=1 turns it on at import.  Returns the previous setting."""
    global BN_INLINE
    L = lib()
    prev = bool(L.saicv_set_deterministic(1 if on else 0))
    if on:
        BN_INLINE = False
        if torch.cuda.is_available():
            check(L.saicv_deterministic_prepare(stream()), 'deterministic_prepare')
    else:
        BN_INLINE = _os.environ.get('SAICV_BN_INLINE', '1') == '1'
    return prev


def is_deterministic():
    return bool(lib().saicv_get_deterministic())


if _os.environ.get('SAICV_DETERMINISTIC') == '1' and _lib.available():
    lib().saicv_set_deterministic(1)          # (the workspace is allocated by the first reduction: no device context at import)
    BN_INLINE = False


class _BnLink:
    """What the data gradient of the NEXT conv needs to produce the backward partial sums of a BatchNorm(+ReLU) node,
    and where that node finds them.  Travels forward as an attribute of the node's output tensor."""
    __slots__ = ('y', 'mask', 'mean', 'invstd', 'part', 'rows', 'dx', 'dx_version', 'inline')

    def __init__(self, y, mask, mean, invstd):
        self.y, self.mask, self.mean, self.invstd = y, mask, mean, invstd
        self.part = self.dx = None
        self.rows = self.dx_version = 0
        self.inline = False


class _GateLedger:
    """Gated shortcut gradients handed out in the running backward and not yet consumed.  A gradient that reaches a
    node that does not know about its gate would silently be used unmasked: the end-of-backward check turns that into
    an error."""
    pending = 0
    queued = False

    @classmethod
    def hand_out(cls):
        cls.pending += 1
        if not cls.queued:
            cls.queued = True
            torch.autograd.Variable._execution_engine.queue_callback(cls._check)

    @classmethod
    def consume(cls):
        cls.pending -= 1

    @classmethod
    def _check(cls):
        n, cls.pending, cls.queued = cls.pending, 0, False
        if n != 0:
            raise RuntimeError(f'{n} gated shortcut gradient(s) did not reach a node that applies the gate (a residual '
                               'tensor with several consumers?); rerun with SAICV_BN_FUSE=0')


def _take_gate(t):
    """ReLU-mask that still has to be applied to gradient tensor t (handed out by a residual node), or None."""
    g = getattr(t, '_saicv_gate', None) if t is not None else None
    if g is not None:
        if t._version != t._saicv_gate_version:
            # autograd summed another gradient into this tensor in place: the gate no longer describes its content
            raise RuntimeError('a gated shortcut gradient was accumulated into before its gate was applied (a residual '
                               'tensor with several consumers); rerun with SAICV_BN_FUSE=0')
        _GateLedger.consume()
        t._saicv_gate = None
    return g


def compute_dtype():
    if torch.is_autocast_enabled('cuda'):
        dt = torch.get_autocast_dtype('cuda')
        if dt != torch.bfloat16:
            raise RuntimeError(f'saicv kernels run bf16 or fp32; autocast dtype {dt} is not supported '
                               '(MI355X perf mode is bf16)')
        return dt
    return torch.float32


def _nhwc(x, dt=None):
    """Returns x as a dense NHWC-strided tensor [of dtype dt] (no copy when it already is)."""
    if x.dim() != 4:
        raise ValueError('expected a 4-d NCHW-shaped tensor')
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    return x if dt is None or x.dtype == dt else x.to(dt)


def _empty_nhwc(n, c, h, w, dtype, device):
    return torch.empty((n, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)


class ResizeBilinearAddFn(torch.autograd.Function):
    """F.interpolate(top, size=lateral.shape[2:], mode='bilinear') + lateral, the top-down merge of a feature pyramid (reference
    SimpleAICV/detection/models/fpn.py:57-75), as one pass over NHWC tensors; fp32 output as under torch.autocast (which runs the
    resize in fp32).  The gradient towards `top` is a gather in a fixed order -- ATen's upsample backward scatters with atomics, the
    one place where a RetinaNet / FCOS step was not reproducible in deterministic mode."""

    @staticmethod
    def forward(ctx, top, lateral):
        require_gpu(top, lateral)
        top, lateral = _nhwc(top), _nhwc(lateral)
        n, c, h, w = top.shape
        _, _, H, W = lateral.shape
        out = _empty_nhwc(n, c, H, W, torch.float32, top.device)
        check(lib().saicv_resize_bilinear_add_fwd(dtype_code(top.dtype), dtype_code(lateral.dtype), ptr(top), ptr(lateral), ptr(out),
                                                  n, h, w, H, W, c, stream()), 'resize_bilinear_add_fwd')
        ctx.geom = (n, c, h, w, H, W, top.dtype, lateral.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        n, c, h, w, H, W, tdt, ldt = ctx.geom
        dout = _nhwc(dout.float())
        dtop = None
        if ctx.needs_input_grad[0]:
            dtop = _empty_nhwc(n, c, h, w, tdt, dout.device)
            check(lib().saicv_resize_bilinear_bwd(dtype_code(tdt), ptr(dout), ptr(dtop), n, h, w, H, W, c, stream()), 'resize_bilinear_bwd')
        return dtop, (dout.to(ldt) if ctx.needs_input_grad[1] else None)


def resize_bilinear_add(top, lateral):
    return ResizeBilinearAddFn.apply(top, lateral)


class ResizeBilinearFn(torch.autograd.Function):
    """F.interpolate(x, size=(H, W), mode='bilinear') on NHWC data: the merge kernel above without a lateral (reference
    SimpleAICV/semantic_segmentation/models/pfan_semantic_segmentation.py:275-295); fp32 output, fixed-order gather backward."""

    @staticmethod
    def forward(ctx, x, H, W):
        require_gpu(x)
        x = _nhwc(x)
        n, c, h, w = x.shape
        out = _empty_nhwc(n, c, H, W, torch.float32, x.device)
        check(lib().saicv_resize_bilinear_add_fwd(dtype_code(x.dtype), _lib.F32, ptr(x), 0, ptr(out), n, h, w, H, W, c, stream()),
              'resize_bilinear_fwd')
        ctx.geom = (n, c, h, w, H, W, x.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        n, c, h, w, H, W, dt = ctx.geom
        dout = _nhwc(dout.float())
        dx = _empty_nhwc(n, c, h, w, dt, dout.device)
        check(lib().saicv_resize_bilinear_bwd(dtype_code(dt), ptr(dout), ptr(dx), n, h, w, H, W, c, stream()), 'resize_bilinear_bwd')
        return dx, None, None


def resize_bilinear(x, size):
    return ResizeBilinearFn.apply(x, int(size[0]), int(size[1]))


_desc_cache = {}


def _desc(N, H, W, C, K, R, S, stride, pad, dt):
    key = (N, H, W, C, K, R, S, stride, pad, dt)
    d = _desc_cache.get(key)
    if d is None:
        OH = (H + 2 * pad - R) // stride + 1
        OW = (W + 2 * pad - S) // stride + 1
        d = ConvDesc(N, H, W, C, K, R, S, stride, pad, OH, OW, dtype_code(dt))
        _desc_cache[key] = d
    return d


# ------------------------------------------------------------------------------ packing
def pack_input(x, dtype=None, cp=8):
    """NCHW-shaped image batch (any strides) -> NHWC compute-dtype tensor with C padded to cp."""
    require_gpu(x)
    if dtype is None:
        dtype = compute_dtype()
    if x.dtype != torch.float32:
        x = x.float()
    n, c, h, w = x.shape
    cp = max(cp, ((c + _lib.epc(dtype) - 1) // _lib.epc(dtype)) * _lib.epc(dtype))
    out = torch.empty((n, h, w, cp), dtype=dtype, device=x.device)
    sn, sc, sh, sw = x.stride()
    check(lib().saicv_pack_input(dtype_code(dtype), ptr(x), sn, sc, sh, sw, ptr(out), n, c, h, w, cp,
                                 stream()), 'pack_input')
    return out.permute(0, 3, 1, 2)


# the convolution + BatchNorm shortcut of a residual block hands its raw output to the block's join, which applies the
# shortcut's BatchNorm in the same pass as the main branch's (one write + one read of the widest tensor of the block less);
# SAICV_DS_JOIN_FUSE=0 materialises the normalised shortcut as before
DS_JOIN_FUSE = _os.environ.get('SAICV_DS_JOIN_FUSE', '1') == '1'
# BatchNorm-apply + ReLU + MaxPool of the ResNet stem as one pass (csrc/pool.hip bn_relu_maxpool_*); 0: the unfused pair
STEM_POOL_FUSE = _os.environ.get('SAICV_STEM_POOL_FUSE', '1') == '1'


def pack_stem_input(x, conv, dtype=None):
    """Input of a stem convolution in the layout its kernel wants: for a K x K stride-2 stem (ResNet: 7 x 7, padding 3,
    reference resnet.py:172-174) the space-to-depth image of saicv_pack_input_s2d -- the convolution then runs as a
    stride-1 (K+1)/2-tap one with 4C (padded to 16) channels, K dimension 256 instead of 392 -- else pack_input()."""
    k = conv.kernel_size[0]
    if (not x.requires_grad and conv.stride == (2, 2) and conv.kernel_size[0] == conv.kernel_size[1] and k % 2 == 1
            and conv.padding == (k // 2, k // 2) and conv.groups == 1 and 4 * x.shape[1] <= 16):
        require_gpu(x)
        dtype = dtype or compute_dtype()
        if x.dtype != torch.float32:
            x = x.float()
        n, c, h, w = x.shape
        pad = k // 2
        hq, wq, cq = (h + 2 * pad + 1) // 2, (w + 2 * pad + 1) // 2, 16
        out = torch.empty((n, hq, wq, cq), dtype=dtype, device=x.device)
        sn, sc, sh, sw = x.stride()
        check(lib().saicv_pack_input_s2d(dtype_code(dtype), ptr(x), sn, sc, sh, sw, ptr(out), n, c, h, w, pad, cq, stream()),
              'pack_input_s2d')
        out = out.permute(0, 3, 1, 2)
        out._saicv_s2d = (c, h, w, k, pad)
        return out
    return pack_input(x, dtype)


def _packed_weight_s2d(weight, dtype, cq):
    """Wf[O][(R+1)/2][(S+1)/2][cq] of a stride-2 stem weight regrouped for the space-to-depth input; cached like packed_weight."""
    key = (weight._version, _weights_epoch[0], dtype, cq, weight.data_ptr())
    cache = getattr(weight, '_saicv_pack_s2d', None)
    if cache is not None and cache[0] == key:
        return cache[1]
    w = weight.detach()
    o, i, r, s = w.shape
    so, si, sr, ss = w.stride()
    wf = torch.empty((o, (r + 1) // 2, (s + 1) // 2, cq), dtype=dtype, device=w.device)
    check(lib().saicv_pack_weight_s2d(dtype_code(dtype), ptr(w), so, si, sr, ss, o, i, r, s, cq, ptr(wf), stream()),
          'pack_weight_s2d')
    weight._saicv_pack_s2d = (key, wf)
    return wf


class _PackRegistry:
    """Compute-dtype copies of every parameter that went through packed_weight(), refreshed by ONE batched launch
    (saicv_pack_weight_batched) the first time one of them is asked for after the optimizer changed the weights, instead of
    one launch per layer and step.  The copies keep their storage, so a captured step replays against the same pointers."""
    entries = {}            # (id(param), dtype, cin_padded, cout_padded) -> dict
    table = None            # (signature, device descriptor tensor, n, total tiles, dtype)
    # Descriptor tables a CAPTURED step launched with.  The graph keeps the table's device ADDRESS; the table itself was built in the
    # eager warm-up (a host -> device copy cannot be captured), i.e. in the ordinary allocator pool -- were it dropped when a later
    # eager step changes the set of live weights (an evaluation between epochs, an EMA model, one eager iteration between replays),
    # the allocator would hand its memory to the next tensor and the replayed launch would read descriptors out of that: wild
    # writes, a GPU memory fault (r05, found by tests/test_gpu_train_loop.py::test_detr_batch_beyond_max_annots_...).  Never freed;
    # one small tensor per capture.
    pinned_tables = []

    @classmethod
    def get(cls, weight, dtype, cin_padded, cout_padded, need_wd, rows=None):
        """rows = (parameter, r0, r1): `weight` is the row block parameter[r0:r1] of a packed parameter (nn.MultiheadAttention's
        in_proj_weight through ops_tfm.linear_rows) -- an entry of its own, refreshed by the same batched launch from the
        parameter's storage (r06: DETR spent 83 single-matrix pack launches per step on them)."""
        import weakref
        base = weight if rows is None else rows[0]
        k = (id(base), None if rows is None else (rows[1], rows[2]), dtype, cin_padded, cout_padded)
        e = cls.entries.get(k)
        if e is not None and e['ref']() is not base:
            e = None                                            # id() reused by another tensor
        if e is None:
            w = weight.detach()
            if w.dim() == 2:
                o, i, r, s = w.shape[0], w.shape[1], 1, 1
            else:
                o, i, r, s = w.shape
            alloc = torch.empty if cout_padded == o else torch.zeros
            e = {'ref': weakref.ref(base), 'rows': None if rows is None else (rows[1], rows[2]), 'dtype': dtype, 'ip': cin_padded, 'op': cout_padded, 'dims': (o, i, r, s),
                 'wf': alloc((cout_padded, r, s, cin_padded), dtype=dtype, device=w.device), 'wd': None, 'key': None, 'used': 0}
            cls.entries[k] = e
            cls.table = None
        if need_wd and e['wd'] is None:
            o, i, r, s = e['dims']
            alloc = torch.empty if cout_padded == o else torch.zeros
            e['wd'] = alloc((i, r, s, cout_padded), dtype=dtype, device=weight.device)
            e['key'] = None                                     # the new matrix has not been filled yet
            cls.table = None
        e['used'] = _weights_epoch[0]
        return e

    @classmethod
    def refresh(cls):
        """One launch over every live entry; stamps each with the key its weight has NOW."""
        live = [(k, e, e['ref']()) for k, e in cls.entries.items()]
        for k, e, w in live:
            if w is None:
                del cls.entries[k]
                cls.table = None
        # weights nobody asked for since the epoch before last (another model of the process) wait until they are wanted
        live = [(k, e, w) for k, e, w in live if w is not None and w.is_cuda and e['used'] >= _weights_epoch[0] - 1]
        # (an entry of a row block packs the view parameter[r0:r1]; its key is stamped with the parameter's version)
        views = {id(e): (w.detach()[e['rows'][0]:e['rows'][1]] if e.get('rows') else w.detach()) for _, e, w in live}
        if not live:
            return
        by_dtype = {}
        for k, e, w in live:
            by_dtype.setdefault(e['dtype'], []).append((e, w))
        sig = tuple((id(e), views[id(e)].data_ptr(), views[id(e)].stride(), ptr(e['wf']), ptr(e['wd'])) for _, e, w in live)
        if cls.table is None or cls.table[0] != sig:
            tables = []
            for dt, items in by_dtype.items():
                arr = (_lib.PackDesc * len(items))()
                t0 = 0
                for j, (e, w) in enumerate(items):
                    o, i, r, s = e['dims']
                    wv = views[id(e)]
                    if wv.dim() == 2:
                        so, si = wv.stride()
                        sr = ss = 0
                    else:
                        so, si, sr, ss = wv.stride()
                    d = arr[j]
                    d.w, d.sO, d.sI, d.sR, d.sS = wv.data_ptr(), so, si, sr, ss
                    d.O, d.I, d.R, d.S, d.Ip, d.Op = o, i, r, s, e['ip'], e['op']
                    d.wf, d.wd = ptr(e['wf']), ptr(e['wd'])
                    # 64 x 64 tiles with 16-byte reads / 8-byte writes where the input-channel axis is contiguous and aligned
                    vec = (si == 1 and all(v % 4 == 0 for v in (so, sr, ss, i, e['ip'], e['op'])) and wv.data_ptr() % 16 == 0)
                    ts = 64 if vec else 32
                    d.tile = ts
                    d.tiles_i, d.tiles_o = (e['ip'] + ts - 1) // ts, (e['op'] + ts - 1) // ts
                    d.tile_begin = t0
                    t0 += d.tiles_i * d.tiles_o * r * s
                dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(items[0][1].device)
                tables.append((dt, dev, len(items), t0))
            cls.table = (sig, tables)
        if live[0][2].is_cuda and torch.cuda.is_current_stream_capturing() and not any(t is cls.table for t in cls.pinned_tables):
            cls.pinned_tables.append(cls.table)
        for dt, dev, n, tiles in cls.table[1]:
            check(lib().saicv_pack_weight_batched(dtype_code(dt), ptr(dev), n, tiles, stream()), 'pack_weight_batched')
        for _, e, w in live:
            e['key'] = (w._version, _weights_epoch[0], views[id(e)].data_ptr())

    @classmethod
    def used_now(cls):
        """The live entries (asked for since the weight change before last -- the rule of refresh()): what a step that has just been
        captured depends on (its own optimizer step has already bumped the epoch once)."""
        return [e for e in cls.entries.values() if e['used'] >= _weights_epoch[0] - 1]

    @classmethod
    def touch(cls, entries):
        """A replayed step used these entries without running get(): keep them among the live ones, so that an eager step between
        replays refreshes the same set through the same descriptor table (engine.StepGraph calls this after every replay)."""
        for e in entries:
            e['used'] = _weights_epoch[0]


def packed_weight(weight, dtype, cin_padded, need_wd, cout_padded=None):
    """Compute-dtype copies of a conv / linear master weight, cached until the weight changes.

    Returns (wf [Op][R][S][Ip], wd [I][R][S][Op] or None); rows/cols beyond O are zero."""
    cout_padded = cout_padded or weight.shape[0]
    rows = getattr(weight, '_saicv_rows_of', None)          # (parameter, r0, r1): ops_tfm.LinearRowsFn
    if weight.is_cuda and (isinstance(weight, torch.nn.Parameter) or rows is not None):
        e = _PackRegistry.get(weight, dtype, cin_padded, cout_padded, need_wd, rows)
        if e['key'] != ((weight if rows is None else rows[0])._version, _weights_epoch[0], weight.data_ptr()):
            _PackRegistry.refresh()
        return e['wf'], (e['wd'] if need_wd else None)
    key = (weight._version, _weights_epoch[0], dtype, cin_padded, cout_padded, weight.data_ptr())
    cache = getattr(weight, '_saicv_pack', None)
    if cache is not None and cache[0] == key and (cache[2] is not None or not need_wd):
        return cache[1], cache[2]
    w = weight.detach()
    if w.dim() == 2:
        o, i = w.shape
        r = s = 1
        so, si = w.stride()
        sr = ss = 0
    else:
        o, i, r, s = w.shape
        so, si, sr, ss = w.stride()
    op = cout_padded
    alloc = torch.empty if op == o else torch.zeros
    wf = alloc((op, r, s, cin_padded), dtype=dtype, device=w.device)
    wd = alloc((i, r, s, op), dtype=dtype, device=w.device) if need_wd else None
    check(lib().saicv_pack_weight(dtype_code(dtype), ptr(w), so, si, sr, ss, o, i, r, s, cin_padded, op,
                                  ptr(wf), ptr(wd), stream()), 'pack_weight')
    weight._saicv_pack = (key, wf, wd)
    return wf, wd


def _weight_grad(dw, weight, cin_padded):
    """fp32 dW[O][R][S][Ip] -> gradient laid out like `weight`."""
    if weight.dim() == 2:
        return dw.view(weight.shape[0], cin_padded)[:, :weight.shape[1]] if cin_padded != weight.shape[1] else dw.view(weight.shape)
    o, i, r, s = weight.shape
    if cin_padded == i and weight.is_contiguous(memory_format=torch.channels_last):
        return dw.permute(0, 3, 1, 2)
    g = torch.empty_strided(weight.shape, weight.stride(), dtype=torch.float32, device=weight.device)
    so, si, sr, ss = g.stride()
    check(lib().saicv_unpack_wgrad(ptr(dw), o, i, r, s, cin_padded, ptr(g), so, si, sr, ss, 0, stream()),
          'unpack_wgrad')
    return g


def _weight_grad_s2d(dw, weight, cq, arena_grad):
    """fp32 dW'[O][(R+1)/2][(S+1)/2][cq] of the space-to-depth stem -> the [O, I, R, S] gradient: added straight into the
    arena gradient when there is one (returns None), else a tensor laid out like `weight`."""
    o, i, r, s = weight.shape
    g = arena_grad if arena_grad is not None else torch.empty_strided(weight.shape, weight.stride(), dtype=torch.float32,
                                                                      device=weight.device)
    so, si, sr, ss = g.stride()
    check(lib().saicv_unpack_wgrad_s2d(ptr(dw), o, i, r, s, cq, ptr(g), so, si, sr, ss, int(arena_grad is not None), stream()),
          'unpack_wgrad_s2d')
    return None if arena_grad is not None else g


# ------------------------------------------------------------------------------ conv + BN + act
class _RunningStats:
    """The running-statistics arguments of the kernels that finalise training-mode BatchNorm statistics (saicv_bn_finalize_fwd,
    saicv_bn_act_fwd_stats, saicv_bn_act_fwd_join), worked out once per call: pointers, or 0 where nothing is tracked."""
    __slots__ = ('mean', 'var', 'momentum', 'eps', 'nbt')

    def __init__(self, bn, track):
        if bn.momentum is None:
            raise NotImplementedError('BatchNorm2d(momentum=None) is not supported')
        track = track and bn.running_mean is not None
        self.mean, self.var = (ptr(bn.running_mean), ptr(bn.running_var)) if track else (0, 0)
        self.momentum, self.eps = float(bn.momentum), float(bn.eps)
        self.nbt = ptr(bn.num_batches_tracked) if track else 0

    def finalize(self, sums, sqs, rows, k, count, gamma, beta, mean, invstd, scale, shift, st):
        """`rows` rows of channel sums / sums of squares -> mean, invstd, scale, shift; running statistics, num_batches_tracked += 1"""
        L = lib()
        ws = torch.empty(L.saicv_bn_ws_floats(k), dtype=torch.float32, device=mean.device)
        check(L.saicv_bn_finalize_fwd(ptr(sums), ptr(sqs), rows, k, float(count), ptr(gamma), ptr(beta), self.mean, self.var,
                                      self.momentum, self.eps, ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ptr(ws), self.nbt,
                                      st), 'bn_finalize_fwd')


def _bn_grad_buffers(gamma, beta, k, dev):
    """-> (dgamma, dbeta, direct_bn): both arena gradients, for the BatchNorm-backward kernels to add into, else two fresh vectors"""
    gg, gb = _arena_grad(gamma), _arena_grad(beta)
    if gg is not None and gb is not None:
        return gg, gb, True
    return torch.empty(k, dtype=torch.float32, device=dev), torch.empty(k, dtype=torch.float32, device=dev), False


def _conv_data_grad(d, dy, weight, wd, x_shape, dt, st, fuse=None, addend=None):
    """dx of the convolution `d` describes: the plain data gradient, + addend in its epilogue, or the fused form `fuse`
    (a _lib.DgradFuse) asks for.  wd = None: the [I][R][S][d.K] weight copy is fetched (packed on first use) here.  st: the
    stream, looked up once per autograd node by its forward / backward (torch.cuda.current_stream() is a ~10 us host call)."""
    n, c, h, w = x_shape
    if wd is None:
        _, wd = packed_weight(weight, dt, c, True, d.K)
    dx = _empty_nhwc(n, c, h, w, dt, dy.device)
    L = lib()
    if fuse is not None:
        check(L.saicv_conv2d_dgrad_fused(ctypes.byref(d), ptr(dy), ptr(wd), ctypes.byref(fuse), ptr(dx), st), 'conv2d_dgrad_fused')
    elif addend is not None:
        check(L.saicv_conv2d_dgrad_add(ctypes.byref(d), ptr(dy), ptr(wd), ptr(addend), ptr(dx), st), 'conv2d_dgrad_add')
    else:
        check(L.saicv_conv2d_dgrad(ctypes.byref(d), ptr(dy), ptr(wd), ptr(dx), st), 'conv2d_dgrad')
    return dx


def _conv_weight_grad(d, dy, x, weight, st, s2d=None, bias_out=None):
    """Weight gradient of the convolution `d` describes -> a gradient for `weight`, or None when the kernel accumulated it
    straight into the arena (_arena_grad).  bias_out: fp32 [d.K] the same launch adds the column sums of dy into.  s2d: the input is
    a space-to-depth image (pack_stem_input).  A `d` whose K is zero-padded beyond the weight's rows (ConvFn) gets [d.K, C, R, S]."""
    c = d.C
    gw = _arena_grad(weight)
    # KRSC fp32 gradient: straight into the arena (atomics accumulate) where its view has that layout row for row -- the ONE rule
    # for "the kernel may accumulate into p.grad", which the engine's "gradient complete" signal relies on -- else a temporary
    direct = (gw is not None and d.K == weight.shape[0] and c == weight.shape[1]
              and weight.is_contiguous(memory_format=torch.channels_last))
    dw = gw if direct else torch.zeros((d.K, d.R, d.S, c), dtype=torch.float32, device=x.device)
    L = lib()
    if bias_out is None:
        check(L.saicv_conv2d_wgrad(ctypes.byref(d), ptr(dy), ptr(x), ptr(dw), st), 'conv2d_wgrad')
    else:
        check(L.saicv_conv2d_wgrad_bias(ctypes.byref(d), ptr(dy), ptr(x), ptr(dw), ptr(bias_out), st), 'conv2d_wgrad')
    if direct:
        return None
    if s2d is not None:
        return _weight_grad_s2d(dw, weight, c, gw)
    if d.K != weight.shape[0]:
        return dw.permute(0, 3, 1, 2)
    return _weight_grad(dw, weight, c)


# what the convolution + statistics stage of ConvBnActFn.forward hands to the tail that follows it (run: _RunningStats or None)
_ConvStage = collections.namedtuple('_ConvStage', 'x y d wd M st training inline stats rows mean invstd scale shift run eps in_link s2d')


def _conv_stage(x, weight, gamma, beta, bn, stride, pad, need_dx, pooled, defer):
    """Input checks, weights and descriptor (space-to-depth or ordinary), the convolution with its BatchNorm statistics, and
    the coefficients where they are needed as tensors: scale / shift in eval mode and, with `inline` false, in training."""
    require_gpu(x, weight)
    # this conv's data gradient IS the dz of the BatchNorm(+ReLU) node that produced x (when x has no other consumer):
    # it can leave that node's backward partial sums behind (the pooled block's data gradient is the plain one)
    in_link = getattr(x, '_saicv_bn', None) if (BN_FUSE and need_dx and not pooled) else None
    xin = x
    x = _nhwc(x)
    dt = x.dtype
    n, c, h, w = x.shape
    k, ci, r, s = weight.shape
    if c < ci:
        raise ValueError(f'input has {c} channels, weight expects {ci}')
    if in_link is not None and not (x is xin and c == ci and in_link.y.shape == x.shape and in_link.y.dtype == dt):
        in_link = None
    s2d = getattr(xin, '_saicv_s2d', None)
    if s2d is not None:
        # stride-2 stem on the space-to-depth image (pack_stem_input): a stride-1 convolution with (R+1)/2 taps
        if need_dx or (s2d[0], s2d[3], s2d[4]) != (ci, r, pad) or stride != 2 or r != s:
            raise ValueError('space-to-depth stem input does not match this convolution')
        wf, wd = _packed_weight_s2d(weight, dt, c), None
        d = _desc(n, h, w, c, k, (r + 1) // 2, (s + 1) // 2, 1, 0, dt)
    else:
        wf, wd = packed_weight(weight, dt, c, need_dx and c == ci)
        d = _desc(n, h, w, c, k, r, s, stride, pad, dt)
    L, st, dev = lib(), stream(), x.device
    y = _empty_nhwc(n, k, d.OH, d.OW, dt, dev)
    M = n * d.OH * d.OW
    training = bn.training
    scale = torch.empty(k, dtype=torch.float32, device=dev)
    shift = torch.empty(k, dtype=torch.float32, device=dev)
    mean = invstd = stats = run = None
    rows = 0
    # (the pooled form takes scale / shift from the finalize kernel: one 6 us launch, stem only)
    atomic_rows = training and BN_INLINE and k <= 2048 and not pooled
    # a deferred apply needs scale / shift as tensors: the finalize launch stays (over the few rows)
    inline = atomic_rows and not defer
    flops = 2.0 * M * k * r * s * min(c, ci)
    if training:
        rows = L.saicv_conv2d_stat_rows(ctypes.byref(d))
        t0 = KernelTimer.begin('igemm_nt')
        if atomic_rows:
            rows = _stat_rows(rows)
            stats = _ZeroPool.take(2 * rows * k, dev).view(2, rows, k)
            check(L.saicv_conv2d_fwd_stats(ctypes.byref(d), ptr(x), ptr(wf), ptr(y), ptr(stats[0]), ptr(stats[1]), rows, st),
                  'conv2d_fwd_stats')
        else:
            stats = torch.empty((2, rows, k), dtype=torch.float32, device=dev)
            check(L.saicv_conv2d_fwd(ctypes.byref(d), ptr(x), ptr(wf), 0, ptr(y), 0, ptr(stats[0]), ptr(stats[1]), st), 'conv2d_fwd')
        es = x.element_size()
        xin_px = M if (r == 1 and stride > 1) else n * h * w          # a strided 1x1 reads a quarter of its input
        KernelTimer.end(t0, 'igemm_nt', flops, float(xin_px) * c * es + float(k) * r * s * c * es + float(M) * k * es)
        mean = torch.empty(k, dtype=torch.float32, device=dev)
        invstd = torch.empty(k, dtype=torch.float32, device=dev)
        run = _RunningStats(bn, bn.track_running_stats)
        if not inline:
            run.finalize(stats[0], stats[1], rows, k, M, gamma, beta, mean, invstd, scale, shift, st)
    else:
        t0 = KernelTimer.begin('igemm_nt')
        check(L.saicv_conv2d_fwd(ctypes.byref(d), ptr(x), ptr(wf), 0, ptr(y), 0, 0, 0, st), 'conv2d_fwd')
        KernelTimer.end(t0, 'igemm_nt', flops, 0)
        check(L.saicv_bn_eval_coeffs(k, ptr(gamma), ptr(beta), ptr(bn.running_mean), ptr(bn.running_var), float(bn.eps),
                                     ptr(scale), ptr(shift), st), 'bn_eval_coeffs')
    return _ConvStage(x, y, d, wd, M, st, training, inline, stats, rows, mean, invstd, scale, shift, run, float(bn.eps), in_link, s2d)


def _remember(ctx, cs, weight, gamma, beta, stride, pad, relu, has_res, mask_or_idx=None, pool=None, gated_res=False, link=None,
              applies_gate=False):
    """Everything ConvBnActFn.backward reads, for every tail of the forward: the saved tensors in the one slot order
    (x, weight, gamma, y, mask_or_idx, mean, invstd_or_scale) and every ctx attribute."""
    # eval-mode backward (frozen statistics) is linear, dy = scale * g: `scale` travels in the slot of invstd, the others stay empty
    last = (mask_or_idx, cs.mean, cs.invstd) if cs.training else (None, None, cs.scale)
    ctx.save_for_backward(cs.x, weight, gamma, cs.y, *last)
    ctx.cfg = (stride, pad, relu, has_res, cs.training, cs.d, cs.wd)
    ctx.in_link, ctx.s2d, ctx.pool, ctx.beta_ref = cs.in_link, cs.s2d, pool, beta
    ctx.gated_res, ctx.link, ctx.applies_gate = gated_res, link, applies_gate


def _pooled_tail(ctx, cs, weight, gamma, beta, stride, pad, pool):
    """BatchNorm-apply + ReLU + MaxPool2d as one pass over the raw convolution output (the ResNet stem)."""
    pk, ps, pp = pool
    y, d = cs.y, cs.d
    n, k = y.shape[0], y.shape[1]
    poh, pow_ = (d.OH + 2 * pp - pk) // ps + 1, (d.OW + 2 * pp - pk) // ps + 1
    zp = _empty_nhwc(n, k, poh, pow_, y.dtype, y.device)
    idx = torch.empty((n, poh, pow_, k), dtype=torch.uint8, device=y.device)
    es = y.element_size()
    # the routed backward (_stem_routed_backward) takes its per-channel sums from the raw y at the recorded maxima: the forward keeps
    # them (pooled size).  The conditions only Python knows come first; no new entry point is fetched without them.  route: bit 0
    # the sums from the kept maxima, bit 1 the stream kernel of csrc/stembwd.hip as well (saicv_stem_bwd_stream_ok)
    ya, route = None, 0
    if y.dtype == torch.bfloat16 and cs.s2d is not None and cs.training and ctx.needs_input_grad[1]:
        route = lib().saicv_stem_bwd_stream_ok(dtype_code(y.dtype), n, d.OH, d.OW, k, d.C, d.R, d.S, pk, ps, pp)
    if route > 0:
        ya = _empty_nhwc(n, k, poh, pow_, y.dtype, y.device)
        t0 = KernelTimer.begin('stem_pool_keep')
        check(lib().saicv_bn_relu_maxpool_fwd_keep(dtype_code(y.dtype), ptr(y), ptr(cs.scale), ptr(cs.shift), ptr(zp), ptr(idx), ptr(ya),
                                                   n, d.OH, d.OW, k, poh, pow_, pk, ps, pp, cs.st), 'bn_relu_maxpool_fwd_keep')
        KernelTimer.end(t0, 'stem_pool_keep', 0, float(cs.M) * k * es + float(n) * poh * pow_ * k * (2 * es + 1))
    else:
        t0 = KernelTimer.begin('bn_act_fwd')
        check(lib().saicv_bn_relu_maxpool_fwd(dtype_code(y.dtype), ptr(y), ptr(cs.scale), ptr(cs.shift), ptr(zp), ptr(idx), n, d.OH, d.OW,
                                              k, poh, pow_, pk, ps, pp, cs.st), 'bn_relu_maxpool_fwd')
        KernelTimer.end(t0, 'bn_act_fwd', 0, float(cs.M) * k * es + float(n) * poh * pow_ * k * (es + 1))
    _remember(ctx, cs, weight, gamma, beta, stride, pad, True, False, idx, (pk, ps, pp, poh, pow_, cs.scale, cs.shift))
    ctx.stem_ya, ctx.stem_route = ya, route
    return zp


def _apply_tail(ctx, cs, weight, gamma, beta, stride, pad, relu, residual, want_skip):
    """BatchNorm-apply [+ residual] [+ ReLU] -> z, by the kernel that fits: bn_act_fwd_join when the residual arrives as a raw
    shortcut convolution + its coefficients, bn_act_fwd_stats when this node's statistics are finalised inline, else bn_act_fwd."""
    res_gate_ok = bool(residual is not None and getattr(residual, '_saicv_gate_ok', False))
    res_affine = getattr(residual, '_saicv_deferred', None) if residual is not None else None
    y, M, run = cs.y, cs.M, cs.run
    dt, dev = y.dtype, y.device
    n, k, oh, ow = y.shape
    if residual is not None:
        res_in = residual
        residual = _nhwc(residual, dt)
        if res_affine is not None and (residual is not res_in or residual.shape != y.shape):
            # not the tensor the coefficients were made for (a layout / dtype change in between): apply them here
            residual = (residual.float() * res_affine[0].view(1, -1, 1, 1) + res_affine[1].view(1, -1, 1, 1)).to(dt)
            residual = _nhwc(residual)
            res_affine = None
    z = _empty_nhwc(n, k, oh, ow, dt, dev)
    # backward needs only the sign of z: one byte per 16-byte chunk instead of re-reading z twice
    mask = (torch.empty(M * k // _lib.epc(dt), dtype=torch.uint8, device=dev)
            if (relu and cs.training and any(ctx.needs_input_grad)) else None)
    L, st = lib(), cs.st
    t0 = KernelTimer.begin('bn_act_fwd')
    if res_affine is not None:
        # the shortcut arrives as a raw convolution output + its BatchNorm coefficients: applied on the fly.  This node's own
        # coefficients come as tensors or, inline, out of the statistics rows (with everything the finalize kernel does)
        if cs.inline:
            own = (0, 0, ptr(cs.stats[0]), ptr(cs.stats[1]), cs.rows)
            upd = (run.mean, run.var, run.momentum, run.eps, run.nbt, ptr(cs.mean), ptr(cs.invstd))
        else:
            own = (ptr(cs.scale), ptr(cs.shift), 0, 0, 0)
            upd = (0, 0, 0.0, cs.eps, 0, 0, 0)
        check(L.saicv_bn_act_fwd_join(dtype_code(dt), ptr(y), ptr(residual), ptr(res_affine[0]), ptr(res_affine[1]), ptr(z), *own,
                                      float(M), ptr(gamma), ptr(beta), *upd, M, k, int(relu), ptr(mask), st), 'bn_act_fwd_join')
    elif cs.inline:
        # the kernel derives mean / invstd / scale / shift from the few statistics rows itself (and updates the running
        # statistics and num_batches_tracked): no finalize launch between the convolution and this one
        check(L.saicv_bn_act_fwd_stats(dtype_code(dt), ptr(y), ptr(residual), ptr(z), ptr(cs.stats[0]), ptr(cs.stats[1]), cs.rows,
                                       float(M), ptr(gamma), ptr(beta), run.mean, run.var, run.momentum, run.eps, run.nbt,
                                       ptr(cs.mean), ptr(cs.invstd), M, k, int(relu), ptr(mask), st), 'bn_act_fwd_stats')
    else:
        check(L.saicv_bn_act_fwd(dtype_code(dt), ptr(y), ptr(residual), ptr(z), ptr(cs.scale), ptr(cs.shift), M, k, int(relu),
                                 ptr(mask), st), 'bn_act_fwd')
    KernelTimer.end(t0, 'bn_act_fwd', 0, float(M) * k * y.element_size() * (3 if residual is not None else 2))
    # the shortcut gradient may come back as (gradient, gate) only from nodes that apply gates: the alias of want_skip
    # (its gradient joins in this node's dgrad epilogue) and BatchNorm nodes without a ReLU of their own
    gated_res = bool(BN_FUSE and res_gate_ok and mask is not None and ctx.needs_input_grad[4] and residual.shape == z.shape)
    # conv_bn_act() below hangs link / applies_gate on the OUTPUT tensors (the objects autograd hands back, not the ones made here)
    link = _BnLink(y, mask, cs.mean, cs.invstd) if (BN_FUSE and mask is not None) else None
    _remember(ctx, cs, weight, gamma, beta, stride, pad, bool(relu), residual is not None, mask, None, gated_res, link,
              bool(BN_FUSE and cs.training and not relu))
    return (z, cs.x) if want_skip else z


def _bn_act_backward(ctx, st, dz, dz_is_given, gate_in, relu, has_res, gamma, y, mask, mean, invstd):
    """dz -> (dy, dres, dgamma, dbeta) behind the BatchNorm-apply [+ residual] [+ ReLU] of the apply tail.  dz_is_given: dz is
    the tensor autograd handed over, not a re-laid-out or cast copy.  gate_in: a ReLU mask that still has to be applied to dz."""
    L = lib()
    dt, dev = y.dtype, y.device
    n, k, oh, ow = y.shape
    M = n * oh * ow
    if gate_in is not None:
        if relu:
            raise RuntimeError('a gated shortcut gradient reached a BatchNorm node with its own ReLU')
        relu, mask = True, gate_in      # same [M][C] coordinates: the tail's mask gates this node's dz
    dy = _empty_nhwc(n, k, oh, ow, dt, dev)
    dres = None
    if has_res and ctx.needs_input_grad[4]:
        if ctx.gated_res and dz_is_given:
            # the masked copy g = dz * [z > 0] is not written: the consumer gets dz and the mask
            dres = dz
            dres._saicv_gate = mask
            dres._saicv_gate_version = dres._version
            _GateLedger.hand_out()
        else:
            dres = _empty_nhwc(n, k, oh, ow, dt, dev)
    dres_out = dres if (dres is not None and dres is not dz) else None
    dgamma, dbeta, direct_bn = _bn_grad_buffers(gamma, ctx.beta_ref, k, dev)
    ws = torch.empty(L.saicv_bn_bwd_ws_floats(M, k, dtype_code(dt)), dtype=torch.float32, device=dev)
    link = ctx.link
    # dz IS the tensor that data gradient wrote (same memory, never written since): with another consumer of z autograd
    # hands over a sum in a different tensor and the three-pass form runs
    fused_reduce = (link is not None and link.part is not None and link.dx is not None and gate_in is None
                    and dz.data_ptr() == link.dx.data_ptr() and dz.shape == link.dx.shape and dz._version == link.dx_version)
    t0 = KernelTimer.begin('bn_act_bwd')
    if fused_reduce and link.inline:
        # ... as a few atomically accumulated rows: coefficients, dgamma and dbeta come out of the one streaming kernel
        check(L.saicv_bn_act_bwd_inline(dtype_code(dt), ptr(dz), ptr(mask), ptr(y), ptr(gamma), ptr(mean), ptr(invstd),
                                        ptr(link.part[0]), ptr(link.part[1]), link.rows, ptr(dy), ptr(dres_out), ptr(dgamma),
                                        ptr(dbeta), M, k, int(relu), int(direct_bn), st), 'bn_act_bwd_inline')
    elif fused_reduce:
        # the data gradient that wrote dz also left the partial sums of this reduction (no pass over dz and y here)
        check(L.saicv_bn_act_bwd_from_partials(dtype_code(dt), ptr(dz), ptr(mask), ptr(y), ptr(gamma), ptr(mean), ptr(invstd),
                                               ptr(link.part[0]), ptr(link.part[1]), link.rows, ptr(dy), ptr(dres_out), ptr(dgamma),
                                               ptr(dbeta), M, k, int(relu), int(direct_bn), ptr(ws), st), 'bn_act_bwd_from_partials')
    else:
        check(L.saicv_bn_act_bwd(dtype_code(dt), ptr(dz), 0, ptr(mask), ptr(y), ptr(gamma), ptr(mean), ptr(invstd),
                                 ptr(dy), ptr(dres_out), ptr(dgamma), ptr(dbeta), M, k, int(relu), int(direct_bn),
                                 ptr(ws), st), 'bn_act_bwd')
    if link is not None:
        link.part = link.dx = None
    # streaming passes over (dz, y) (+ the 1-bit ReLU mask): reduction unless fused away, then apply; dy (and dres) written
    KernelTimer.end(t0, 'bn_act_bwd', 0, float(M) * k * y.element_size() *
                    ((1 if fused_reduce else 2) * (2 + (1.0 / 16 if relu else 0)) + (2 if dres_out is not None else 1)))
    return (dy, dres, None, None) if direct_bn else (dy, dres, dgamma, dbeta)


def _dgrad_fuse(d, in_link, addend, gate, dev):
    """The epilogue of a fused data gradient (_lib.DgradFuse): + addend [* gate], and / or the backward partial sums of the
    BatchNorm(+ReLU) node behind `in_link`, parked on the link for that node's backward."""
    fuse = _lib.DgradFuse()
    fuse.addend, fuse.addend_gate = ptr(addend), ptr(gate)
    if in_link is not None:
        c = d.C
        rows = lib().saicv_conv2d_dgrad_stat_rows(ctypes.byref(d))
        in_link.inline = BN_INLINE and c <= 2048
        if in_link.inline:
            rows = _stat_rows(rows)
            part = _ZeroPool.take(2 * rows * c, dev).view(2, rows, c)
            fuse.part_rows = rows
        else:
            part = torch.empty((2, rows, c), dtype=torch.float32, device=dev)
        fuse.bn_y, fuse.bn_mask = ptr(in_link.y), ptr(in_link.mask)
        fuse.bn_mean, fuse.bn_invstd = ptr(in_link.mean), ptr(in_link.invstd)
        fuse.part_g, fuse.part_gx = ptr(part[0]), ptr(part[1])
        in_link.part, in_link.rows = part, rows
    return fuse


def _pooled_bn_backward(ctx, st, dz, gamma, y, idx, mean, invstd):
    """The pooled stem block's half of backward: pooled gradient -> (max-pool backward + ReLU gate + BatchNorm backward in two
    passes over y) -> (dy at full resolution, no dres, dgamma, dbeta); ConvBnActFn.backward goes on from dy as behind its own kernels."""
    pk, ps, pp, poh, pow_, scale, shift = ctx.pool
    L = lib()
    dt, dev = y.dtype, y.device
    n, k, oh, ow = y.shape
    dy = _empty_nhwc(n, k, oh, ow, dt, dev)
    dgamma, dbeta, direct_bn = _bn_grad_buffers(gamma, ctx.beta_ref, k, dev)
    ws = torch.empty(L.saicv_bn_relu_maxpool_bwd_ws_floats(k), dtype=torch.float32, device=dev)
    t0 = KernelTimer.begin('bn_act_bwd')
    check(L.saicv_bn_relu_maxpool_bwd(dtype_code(dt), ptr(dz), ptr(idx), ptr(y), ptr(gamma), ptr(mean), ptr(invstd), ptr(scale),
                                      ptr(shift), ptr(dy), ptr(dgamma), ptr(dbeta), int(direct_bn), ptr(ws), n, oh, ow, k, poh, pow_,
                                      pk, ps, pp, st), 'bn_relu_maxpool_bwd')
    es = y.element_size()
    KernelTimer.end(t0, 'bn_act_bwd', 0, 3.0 * n * oh * ow * k * es + 2.0 * n * poh * pow_ * k * (es + 1))  # y twice + dy; dout + idx twice
    return (dy, None, None, None) if direct_bn else (dy, None, dgamma, dbeta)


def _stem_routed_backward(ctx, st, dz, x, weight, gamma, y, idx, mean, invstd):
    """The pooled space-to-depth stem's backward when its forward kept the maxima (_pooled_tail, ctx.stem_route): the two per-channel
    sums from pooled-size tensors (no pass over y), then either the second pass of the two-kernel backward and the weight gradient as
    before (bit 0 alone), or BatchNorm-backward apply + weight gradient as one stream, csrc/stembwd.hip -- dy is never allocated
    (bit 1).  unpack_wgrad_s2d is the last launch either way.  -> ConvBnActFn.backward's return tuple."""
    pk, ps, pp, poh, pow_, scale, shift = ctx.pool
    d = ctx.cfg[5]
    L = lib()
    dt, dev = y.dtype, y.device
    n, k, oh, ow = y.shape
    c = x.shape[1]
    es = y.element_size()
    pooled = float(n) * poh * pow_ * k
    dgamma, dbeta, direct_bn = _bn_grad_buffers(gamma, ctx.beta_ref, k, dev)
    sums = torch.empty(2 * k, dtype=torch.float32, device=dev)
    t0 = KernelTimer.begin('stem_bwd_sums')
    check(L.saicv_bn_relu_maxpool_bwd_sums(dtype_code(dt), ptr(dz), ptr(ctx.stem_ya), ptr(mean), ptr(invstd), ptr(scale), ptr(shift),
                                           ptr(sums), n, poh, pow_, k, st), 'bn_relu_maxpool_bwd_sums')
    KernelTimer.end(t0, 'stem_bwd_sums', 0, 2.0 * pooled * es)                  # dout + ya
    flops = 2.0 * n * oh * ow * k * d.R * d.S * c
    if ctx.stem_route & 2:
        ws = torch.empty(L.saicv_stem_bwd_stream_ws_floats(n, oh, ow), dtype=torch.float32, device=dev)
        dw = torch.zeros((k, d.R, d.S, c), dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('stem_bwd_stream')
        check(L.saicv_stem_bwd_stream(dtype_code(dt), ptr(dz), ptr(idx), ptr(y), ptr(gamma), ptr(mean), ptr(invstd), ptr(scale),
                                      ptr(shift), ptr(sums), ptr(x), ptr(dw), ptr(dgamma), ptr(dbeta), int(direct_bn), ptr(ws), n, oh, ow,
                                      k, c, d.R, d.S, pk, ps, pp, st), 'stem_bwd_stream')
        # y, dout + idx, the space-to-depth image: each once
        KernelTimer.end(t0, 'stem_bwd_stream', flops, float(n) * oh * ow * k * es + pooled * (es + 1) + float(x.numel()) * es)
        dwt = _weight_grad_s2d(dw, weight, c, _arena_grad(weight))
    else:
        dy = _empty_nhwc(n, k, oh, ow, dt, dev)
        t0 = KernelTimer.begin('stem_bwd_apply')
        check(L.saicv_bn_relu_maxpool_bwd_apply(dtype_code(dt), ptr(dz), ptr(idx), ptr(y), ptr(gamma), ptr(mean), ptr(invstd), ptr(scale),
                                                ptr(shift), ptr(sums), ptr(dy), ptr(dgamma), ptr(dbeta), int(direct_bn), n, oh, ow, k, poh,
                                                pow_, pk, ps, pp, st), 'bn_relu_maxpool_bwd_apply')
        KernelTimer.end(t0, 'stem_bwd_apply', 0, 2.0 * n * oh * ow * k * es + pooled * (es + 1))      # y + dy; dout + idx
        t0 = KernelTimer.begin('igemm_tn')
        dwt = _conv_weight_grad(d, dy, x, weight, st, ctx.s2d)
        KernelTimer.end(t0, 'igemm_tn', flops, 0)
    if direct_bn:
        dgamma = dbeta = None
    return (None, dwt, dgamma if ctx.needs_input_grad[2] else None, dbeta if ctx.needs_input_grad[3] else None, None,
            None, None, None, None, None, None, None)


def _c3_fused_backward(ctx, st, dz, dz_is_given, gate_in, dskip, x, weight, gamma, y, mask, mean, invstd):
    """The whole backward of a bottleneck block's third convolution (1 x 1, stride 1, behind BatchNorm + residual + ReLU) as one
    stream, csrc/c3bwd.hip: finalize launch (coefficients, dgamma, dbeta), then BatchNorm-backward apply + data gradient + weight
    gradient in one kernel -- dy is never allocated -- then the fold.  -> ConvBnActFn.backward's return tuple, or None when the
    node does not qualify (everything else takes the three-kernel path untouched): bf16; the shortcut gradient leaves gated (dres
    is dz, nothing to write); the backward sums came from the data gradient that produced dz; input and weight both want gradients."""
    stride, pad, relu, has_res, training, d, wd = ctx.cfg
    dt = y.dtype
    if not (BN_FUSE and dt == torch.bfloat16 and relu and has_res and mask is not None and gate_in is None and dskip is None
            and dz_is_given and ctx.s2d is None and (d.R, d.S, d.stride, d.pad) == (1, 1, 1, 0)
            and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and (ctx.gated_res or not ctx.needs_input_grad[4])):
        return None
    link = ctx.link
    if not (link is not None and link.part is not None and link.dx is not None and dz.data_ptr() == link.dx.data_ptr()
            and dz.shape == link.dx.shape and dz._version == link.dx_version):
        return None
    n, k, oh, ow = y.shape
    c = x.shape[1]
    M = n * oh * ow
    if c != weight.shape[1] or tuple(x.shape) != (n, c, oh, ow) or x.dtype != dt:
        return None
    L, dev = lib(), y.device
    rows = L.saicv_c3_bwd_stream_ok(dtype_code(dt), M, k, c)
    if rows <= 0:
        return None
    dres = None
    if ctx.needs_input_grad[4]:
        dres = dz                           # the masked copy is not written: the consumer gets dz and the mask
        dres._saicv_gate = mask
        dres._saicv_gate_version = dres._version
        _GateLedger.hand_out()
    dgamma, dbeta, direct_bn = _bn_grad_buffers(gamma, ctx.beta_ref, k, dev)
    ws = torch.empty(L.saicv_c3_bwd_stream_ws_floats(M, k, c), dtype=torch.float32, device=dev)
    if wd is None:
        _, wd = packed_weight(weight, dt, c, True, d.K)
    in_link = ctx.in_link
    fuse = None
    if in_link is not None:                 # the backward sums of the BatchNorm(+ReLU) node that produced x, over the stored dx
        fuse = _lib.DgradFuse()
        in_link.inline = BN_INLINE and c <= 2048
        if in_link.inline:
            prow = _stat_rows(rows)
            part = _ZeroPool.take(2 * prow * c, dev).view(2, prow, c)
            fuse.part_rows = prow
        else:
            prow = rows
            part = torch.empty((2, rows, c), dtype=torch.float32, device=dev)
        fuse.bn_y, fuse.bn_mask = ptr(in_link.y), ptr(in_link.mask)
        fuse.bn_mean, fuse.bn_invstd = ptr(in_link.mean), ptr(in_link.invstd)
        fuse.part_g, fuse.part_gx = ptr(part[0]), ptr(part[1])
        in_link.part, in_link.rows = part, prow
    dx = _empty_nhwc(n, c, oh, ow, dt, dev)
    gw = _arena_grad(weight)
    direct = (gw is not None and d.K == weight.shape[0] and weight.is_contiguous(memory_format=torch.channels_last))
    dw = gw if direct else torch.zeros((k, 1, 1, c), dtype=torch.float32, device=dev)
    t0 = KernelTimer.begin('c3_bwd_stream')
    check(L.saicv_c3_bwd_stream(dtype_code(dt), ptr(dz), ptr(mask), ptr(y), ptr(gamma), ptr(mean), ptr(invstd), ptr(link.part[0]),
                                ptr(link.part[1]), link.rows, ptr(dgamma), ptr(dbeta), int(direct_bn), ptr(ws), ptr(x), ptr(wd),
                                ctypes.byref(fuse) if fuse is not None else None, ptr(dx), ptr(dw), M, k, c, st), 'c3_bwd_stream')
    # both products; dz, y, x, the c2 node's y and dx: 2.75 passes over an [M][k] tensor at c = k / 4
    KernelTimer.end(t0, 'c3_bwd_stream', 2 * 2.0 * M * k * c, 2.75 * M * k * y.element_size())
    link.part = link.dx = None
    if in_link is not None:
        in_link.dx, in_link.dx_version = dx, dx._version
    dwt = None if direct else _weight_grad(dw, weight, c)
    if direct_bn:
        dgamma = dbeta = None
    return (dx, dwt, dgamma if ctx.needs_input_grad[2] else None, dbeta if ctx.needs_input_grad[3] else None, dres,
            None, None, None, None, None, None, None)


class ConvBnActFn(torch.autograd.Function):
    """conv -> [BatchNorm2d (train: batch stats, eval: running stats)] -> [+residual] -> [ReLU].

    Mirrors reference ConvBnActBlock (classification/backbones/resnet.py:19-48) plus the
    residual tail of BasicBlock / Bottleneck (:94-95, :152-153)."""

    # return channel of a deferred forward to conv_bn_act (a tensor attribute set inside forward does not survive apply(), and
    # under no_grad there is no grad_fn to carry it): forward pushes (scale, shift) right before it returns, conv_bn_act pops
    _deferred = []

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, bn, stride, pad, relu, want_skip=False, pool=None, defer=False):
        """defer: the node is the convolution + BatchNorm shortcut of a residual block; it returns the RAW convolution output
        tagged with its BatchNorm coefficients (conv_bn_act hangs `_saicv_deferred` on it) and the one consumer -- the join node
        that takes it as `residual` -- applies them in its own pass (csrc/bn.hip bn_act_fwd_join).  The gradient that comes back
        is the one of the normalised shortcut, so the backward below is the ordinary one.
        pool = (kernel, stride, padding): the MaxPool2d behind the block runs in the same pass as BatchNorm-apply + ReLU
        (the ResNet stem; csrc/pool.hip bn_relu_maxpool_*), the full-resolution activation is never written.
        want_skip: also return the (NHWC) input as a second output.  A residual block routes its shortcut
        through that alias, so the shortcut's gradient reaches THIS node's backward and is added in the
        dgrad kernel's epilogue instead of by a separate elementwise add."""
        if defer and (residual is not None or relu or want_skip or pool is not None):
            raise ValueError('a deferred BatchNorm-apply belongs to a plain convolution + BatchNorm shortcut')
        if pool is not None and (residual is not None or not relu or want_skip):
            raise ValueError('the fused max-pool follows a plain conv -> BatchNorm -> ReLU block')
        cs = _conv_stage(x, weight, gamma, beta, bn, stride, pad, ctx.needs_input_grad[0], pool is not None, defer)
        if pool is not None:
            return _pooled_tail(ctx, cs, weight, gamma, beta, stride, pad, pool)
        if defer:
            # the raw output; its gradient is the normalised shortcut's and may arrive gated (no ReLU of its own)
            _remember(ctx, cs, weight, gamma, beta, stride, pad, False, False, applies_gate=bool(BN_FUSE and cs.training))
            ConvBnActFn._deferred.append((cs.scale, cs.shift))
            return cs.y
        return _apply_tail(ctx, cs, weight, gamma, beta, stride, pad, relu, residual, want_skip)

    @staticmethod
    def backward(ctx, dz, dskip=None):
        x, weight, gamma, y, mask, mean, invstd = ctx.saved_tensors
        stride, pad, relu, has_res, training, d, wd = ctx.cfg
        if not training:
            raise NotImplementedError('backward through eval-mode BatchNorm is not implemented')
        dt, st = y.dtype, stream()
        gate_in = _take_gate(dz)          # dz is a shortcut gradient still waiting for the ReLU mask of the block's tail
        dz0 = dz
        dz = _nhwc(dz, dt)
        if ctx.pool is None:
            fused = _c3_fused_backward(ctx, st, dz, dz is dz0, gate_in, dskip, x, weight, gamma, y, mask, mean, invstd)
            if fused is not None:
                return fused
        if ctx.pool is not None and ctx.stem_route > 0:
            return _stem_routed_backward(ctx, st, dz, x, weight, gamma, y, mask, mean, invstd)
        if ctx.pool is not None:
            dy, dres, dgamma, dbeta = _pooled_bn_backward(ctx, st, dz, gamma, y, mask, mean, invstd)
        else:
            dy, dres, dgamma, dbeta = _bn_act_backward(ctx, st, dz, dz is dz0, gate_in, relu, has_res, gamma, y, mask, mean, invstd)
        n, k, oh, ow = y.shape
        M = n * oh * ow
        c = x.shape[1]
        flops = 2.0 * M * k * weight.shape[2] * weight.shape[3] * min(c, weight.shape[1])
        dx = dwt = None
        if ctx.needs_input_grad[0]:
            t0 = KernelTimer.begin('igemm_nt')
            gate = None
            if dskip is not None:           # gradient of the shortcut alias joins in the dgrad epilogue
                gate = _take_gate(dskip)
                dskip = _nhwc(dskip, dt)
            in_link = ctx.in_link
            fuse = _dgrad_fuse(d, in_link, dskip, gate, y.device) if (gate is not None or in_link is not None) else None
            dx = _conv_data_grad(d, dy, weight, wd, x.shape, dt, st, fuse, dskip)
            if in_link is not None:
                in_link.dx, in_link.dx_version = dx, dx._version
            es = dy.element_size()
            px = float(n) * x.shape[2] * x.shape[3] * c          # elements of dx (and of every epilogue tensor)
            nbytes = float(M) * k * es + float(k) * d.R * d.S * c * es + px * es
            if dskip is not None:
                nbytes += px * es + (px / 8 if gate is not None else 0)
            if in_link is not None:
                nbytes += px * es + px / 8
            KernelTimer.end(t0, 'igemm_nt', flops, nbytes if ctx.pool is None else 0)
        if ctx.needs_input_grad[1]:
            t0 = KernelTimer.begin('igemm_tn')
            dwt = _conv_weight_grad(d, dy, x, weight, st, ctx.s2d)
            KernelTimer.end(t0, 'igemm_tn', flops, 0)
        return (dx, dwt, dgamma if ctx.needs_input_grad[2] else None,
                dbeta if ctx.needs_input_grad[3] else None, dres, None, None, None, None, None, None, None)


def conv_bn_act(x, weight, bn, stride, pad, relu, residual=None, want_skip=False, pool=None, defer=False):
    """defer=True: ONLY for a tensor whose single consumer is the `residual` argument of another conv_bn_act call (what comes
    back is the raw convolution output; its values are not the block's output until that consumer applies the coefficients)."""
    # as conv2d below: under autocast the block's convolution computes in the autocast dtype whatever its input's dtype
    if torch.is_autocast_enabled('cuda') and x.is_floating_point() and x.dtype != compute_dtype() and getattr(x, '_saicv_s2d', None) is None:
        x = x.to(compute_dtype())
    if pool is not None:
        return ConvBnActFn.apply(x, weight, bn.weight, bn.bias, None, bn, stride, pad, relu, False, pool)
    if defer:
        out = ConvBnActFn.apply(x, weight, bn.weight, bn.bias, None, bn, stride, pad, False, False, None, True)
        out._saicv_deferred = ConvBnActFn._deferred.pop()
        if BN_FUSE and out.grad_fn is not None and getattr(out.grad_fn, 'applies_gate', False):
            out._saicv_gate_ok = True
        return out
    out = ConvBnActFn.apply(x, weight, bn.weight, bn.bias, residual, bn, stride, pad, relu, want_skip)
    z = out[0] if want_skip else out
    node = z.grad_fn
    if BN_FUSE and node is not None and hasattr(node, 'link'):
        if node.link is not None:
            z._saicv_bn = node.link            # the next conv's data gradient can do this node's backward reduction
        if node.applies_gate:
            z._saicv_gate_ok = True            # as a residual, its gradient may arrive as (dz, ReLU mask)
        if want_skip:
            out[1]._saicv_gate_ok = True       # the alias: its gradient joins in this node's dgrad epilogue
    return out


# ------------------------------------------------------------------------------ plain conv / linear
class ConvFn(torch.autograd.Function):
    """nn.Conv2d (optional bias, no normalisation) on NHWC data: SAM neck convs (reference
    interactive_segmentation/models/segment_anything/image_encoder.py:303-316), DETR input
    projection (reference detection/models/detr.py:301)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad):
        require_gpu(x, weight)
        x = _nhwc(x)
        dt = x.dtype
        n, c, h, w = x.shape
        k, ci, r, s = weight.shape
        if c != ci and not (c > ci and c - ci < 8 and not ctx.needs_input_grad[0]):
            # c > ci: an image batch zero-padded to whole chunks by pack_input() (stems; no input gradient)
            raise ValueError(f'input has {c} channels, weight expects {ci}')
        need_dx = ctx.needs_input_grad[0]
        wf, wd = packed_weight(weight, dt, c, need_dx)
        d = _desc(n, h, w, c, k, r, s, stride, pad, dt)
        y = _empty_nhwc(n, k, d.OH, d.OW, dt, x.device)
        t0 = KernelTimer.begin('igemm_nt')
        check(lib().saicv_conv2d_fwd(ctypes.byref(d), ptr(x), ptr(wf), ptr(bias), ptr(y), 0, 0, 0, stream()),
              'conv2d_fwd')
        KernelTimer.end(t0, 'igemm_nt', 2.0 * n * d.OH * d.OW * k * r * s * c, 0)
        ctx.save_for_backward(x, weight, bias)
        ctx.cfg = (d, wd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        d, wd = ctx.cfg
        dt, st = x.dtype, stream()
        dy = _nhwc(dy, dt)
        n, c, h, w = x.shape
        k = weight.shape[0]
        e = _lib.epc(dt)
        dx = dwt = db = None
        if k % e:
            # output channels that are not whole 16-byte chunks (RetinaNet's 9 x 4 box offsets, FCOS's 4 + 1 outputs): the
            # backward kernels gather dY by chunks, so dY travels zero-padded to kp channels and the gradients are sliced back
            # (the padded descriptor keeps the weight gradient out of the arena: _conv_weight_grad)
            kp = (k + e - 1) // e * e
            dyp = torch.zeros((n, kp, d.OH, d.OW), dtype=dt, device=dy.device).contiguous(memory_format=torch.channels_last)
            dyp[:, :k] = dy
            dp = _desc(n, h, w, c, kp, d.R, d.S, d.stride, d.pad, dt)
            if ctx.needs_input_grad[0]:
                dx = _conv_data_grad(dp, dyp, weight, None, x.shape, dt, st)
            if ctx.needs_input_grad[1]:
                dwt = _conv_weight_grad(dp, dyp, x, weight, st)[:k].to(weight.dtype)
            if bias is not None and ctx.needs_input_grad[2]:
                # one column sum over the [pixels, k] view of the NHWC gradient, fp32 accumulation without an fp32 copy.  At a
                # million pixels and 151 classes this ATen reduction is the largest kernel of the segmentation step (16.1 ms of
                # 26.1 ms; saicv_colsum on dyp does it in a step of 10.1 ms): DESIGN.md section 3m has the numbers and why it stays
                db = torch.sum(dy.permute(0, 2, 3, 1).reshape(-1, k), dim=0, dtype=torch.float32).to(bias.dtype)
            return dx, dwt, db, None, None
        M = n * d.OH * d.OW
        flops = 2.0 * M * k * d.R * d.S * c
        if ctx.needs_input_grad[0]:
            t0 = KernelTimer.begin('igemm_nt')
            dx = _conv_data_grad(d, dy, weight, wd, x.shape, dt, st)
            KernelTimer.end(t0, 'igemm_nt', flops, 0)
        want_b = bias is not None and ctx.needs_input_grad[2]
        tb = gb = None
        if want_b:
            gb = _arena_grad(bias)
            tb = gb if gb is not None else torch.zeros(k, dtype=torch.float32, device=x.device)
        if ctx.needs_input_grad[1]:
            t0 = KernelTimer.begin('igemm_tn')
            # the bias gradient rides along: column sums of the dY tiles the weight-gradient kernel already holds
            dwt = _conv_weight_grad(d, dy, x, weight, st, None, tb)
            KernelTimer.end(t0, 'igemm_tn', flops, 0)
        elif want_b:                            # no weight gradient wanted: its own pass
            check(lib().saicv_colsum(dtype_code(dt), ptr(dy), M, k, ptr(tb), st), 'colsum')
        if gb is None:
            db = tb
        return dx, dwt, db, None, None


def conv2d(x, weight, bias=None, stride=1, pad=0):
    # under autocast a convolution computes in the autocast dtype whatever its input's dtype (torch.autocast casts conv2d's
    # operands): an fp32 activation -- e.g. the output of a bilinear resize, which autocast runs in fp32 -- is cast here
    if torch.is_autocast_enabled('cuda') and x.is_floating_point() and x.dtype != compute_dtype():
        x = x.to(compute_dtype())
    return ConvFn.apply(x, weight, bias, stride, pad)


class DepthwiseConvFn(torch.autograd.Function):
    """nn.Conv2d(C, C, k, stride, padding, dilation, groups=C) on NHWC data (csrc/dwconv.hip): the depthwise layers of
    reference classification/backbones/van.py:30,68,75 and convformer.py.  weight [C, 1, k, k]; HBM-bound streaming kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, dilation):
        require_gpu(x, weight)
        x = _nhwc(x)
        dt = x.dtype
        n, c, h, w = x.shape
        if weight.shape[0] != c or weight.shape[1] != 1 or weight.shape[2] != weight.shape[3]:
            raise ValueError(f'depthwise weight {tuple(weight.shape)} for {c} channels')
        k = weight.shape[2]
        oh = (h + 2 * pad - dilation * (k - 1) - 1) // stride + 1
        ow = (w + 2 * pad - dilation * (k - 1) - 1) // stride + 1
        wt = weight.detach().reshape(c, k * k).t().contiguous().to(dt)        # tap-major [k*k][C]
        y = _empty_nhwc(n, c, oh, ow, dt, x.device)
        bf = bias.detach().float() if bias is not None else None
        t0 = KernelTimer.begin('dwconv_fwd')
        check(lib().saicv_dwconv2d_fwd(dtype_code(dt), ptr(x), ptr(wt), ptr(bf), ptr(y), n, h, w, c, oh, ow, k, stride, pad, dilation,
                                       stream()), 'dwconv2d_fwd')
        KernelTimer.end(t0, 'dwconv_fwd', 2.0 * n * oh * ow * c * k * k, float(n) * (h * w + oh * ow) * c * x.element_size())
        ctx.save_for_backward(x, weight, bias, wt)
        ctx.cfg = (n, h, w, c, oh, ow, k, stride, pad, dilation)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, wt = ctx.saved_tensors
        n, h, w, c, oh, ow, k, stride, pad, dilation = ctx.cfg
        L, st = lib(), stream()
        dt = x.dtype
        dy = _nhwc(dy, dt)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _empty_nhwc(n, c, h, w, dt, x.device)
            check(L.saicv_dwconv2d_dgrad(dtype_code(dt), ptr(dy), ptr(wt), ptr(dx), n, h, w, c, oh, ow, k, stride, pad, dilation, st),
                  'dwconv2d_dgrad')
        want_b = bias is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            dwt = torch.zeros((k * k, c), dtype=torch.float32, device=x.device)
            tb = torch.zeros(c, dtype=torch.float32, device=x.device) if want_b else None
            check(L.saicv_dwconv2d_wgrad(dtype_code(dt), ptr(dy), ptr(x), ptr(dwt), ptr(tb), n, h, w, c, oh, ow, k, stride, pad, dilation,
                                         st), 'dwconv2d_wgrad')
            if ctx.needs_input_grad[1]:
                dw = dwt.t().reshape(c, 1, k, k).to(weight.dtype)
            db = tb.to(bias.dtype) if want_b else None
        return dx, dw, db, None, None, None


def depthwise_conv2d(x, weight, bias=None, stride=1, pad=0, dilation=1):
    if torch.is_autocast_enabled('cuda') and x.is_floating_point() and x.dtype != compute_dtype():
        x = x.to(compute_dtype())
    return DepthwiseConvFn.apply(x, weight, bias, stride, pad, dilation)


# ------------------------------------------------------------------------------ streaming glue (csrc/elemwise.hip)
ACT_KINDS = {'relu': 0, 'leakyrelu': 1, 'silu': 2}


def _dense(x):
    """x as a dense tensor whose memory order the elementwise kernels may walk: NHWC for 4-d tensors, row-major otherwise."""
    return _nhwc(x) if x.dim() == 4 else x.contiguous()


def _like(x, other):
    """`other` in x's dtype and dense layout"""
    other = _dense(other)
    return other if other.dtype == x.dtype else other.to(x.dtype)


class ActFn(torch.autograd.Function):
    """nn.ReLU / nn.LeakyReLU(slope) / nn.SiLU as one streaming pass (reference darknet.py:16-33, van.py:44,103,
    convformer.py:53,86).  The forward input is kept for the backward (dx = dy * act'(x))."""

    @staticmethod
    def forward(ctx, x, kind, slope):
        require_gpu(x)
        x = _dense(x)
        y = torch.empty_like(x)
        check(lib().saicv_act_fwd(dtype_code(x.dtype), kind, float(slope), ptr(x), ptr(y), x.numel(), stream()), 'act_fwd')
        ctx.save_for_backward(x)
        ctx.cfg = (kind, float(slope))
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        kind, slope = ctx.cfg
        dy = _like(x, dy)
        dx = torch.empty_like(x)
        check(lib().saicv_act_bwd(dtype_code(x.dtype), kind, slope, ptr(dy), ptr(x), ptr(dx), x.numel(), stream()), 'act_bwd')
        return dx, None, None


def act(x, kind, slope=0.):
    return ActFn.apply(x, ACT_KINDS[kind], slope)


class MulFn(torch.autograd.Function):
    """a * b of two activations of one shape (reference van.py:91)."""

    @staticmethod
    def forward(ctx, a, b):
        require_gpu(a, b)
        a = _dense(a)
        b = _like(a, b)
        out = torch.empty_like(a)
        check(lib().saicv_mul_fwd(dtype_code(a.dtype), ptr(a), ptr(b), ptr(out), a.numel(), stream()), 'mul_fwd')
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        dy = _like(a, dy)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(a) if ctx.needs_input_grad[1] else None
        check(lib().saicv_mul_bwd(dtype_code(a.dtype), ptr(dy), ptr(a), ptr(b), ptr(da), ptr(db), a.numel(), stream()), 'mul_bwd')
        return da, db


def mul(a, b):
    return MulFn.apply(a, b)


class ScaleAddFn(torch.autograd.Function):
    """x + s[c] * y on NHWC activations, s a per-channel parameter ([C] after flattening; None: plain x + y): the layer-scaled
    residual of reference van.py:181-185 and the residual joins of darknet.py / convformer.py:157-163."""

    @staticmethod
    def forward(ctx, x, y, s):
        require_gpu(x, y)
        y = _nhwc(y)
        x = _like(y, x) if x is not None else None            # None: s[c] * y alone (a layer scale outside a residual join)
        n, c, h, w = y.shape
        sf = s.detach().reshape(-1).float().contiguous() if s is not None else None
        if sf is not None and sf.numel() != c:
            raise ValueError(f'scale of {sf.numel()} values for {c} channels')
        out = torch.empty_like(y)
        check(lib().saicv_channel_scale_add_fwd(dtype_code(y.dtype), ptr(x), ptr(y), ptr(sf), ptr(out), n * h * w, c, stream()),
              'channel_scale_add_fwd')
        ctx.save_for_backward(y if (s is not None and ctx.needs_input_grad[2]) else None, sf, s)
        ctx.cfg = (n, c, h, w, y.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, sf, s = ctx.saved_tensors
        n, c, h, w, dt = ctx.cfg
        dout = _nhwc(dout, dt)
        dx = dout if ctx.needs_input_grad[0] else None        # (needs_input_grad[0] is False for x = None)
        if s is None:
            return dx, (dout if ctx.needs_input_grad[1] else None), None
        dy = torch.empty_like(dout) if ctx.needs_input_grad[1] else None
        ds = torch.zeros(c, dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[2] else None
        check(lib().saicv_channel_scale_add_bwd(dtype_code(dt), ptr(dout), ptr(y), ptr(sf), ptr(dy), ptr(ds), n * h * w, c, stream()),
              'channel_scale_add_bwd')
        return dx, dy, (ds.reshape(s.shape).to(s.dtype) if ds is not None else None)


def scale_add(x, y, s=None):
    return ScaleAddFn.apply(x, y, s)


class SampleScaleFn(torch.autograd.Function):
    """x[n] * w[n] on an NHWC activation, w fp32 [N]: stochastic depth of a convolutional residual branch (reference van.py:
    118-150, convformer.py:99-131 DropPathBlock).  The same kernel both ways (saicv_row_scale over [N*H*W][C] rows)."""

    @staticmethod
    def forward(ctx, x, w):
        require_gpu(x, w)
        x = _nhwc(x)
        n, c, h, wd = x.shape
        w = w.detach().reshape(-1).float().contiguous()
        out = torch.empty_like(x)
        check(lib().saicv_row_scale(dtype_code(x.dtype), ptr(x), ptr(w), ptr(out), n * h * wd, c, h * wd, stream()), 'row_scale')
        ctx.save_for_backward(w)
        return out

    @staticmethod
    def backward(ctx, dout):
        (w,) = ctx.saved_tensors
        dout = _nhwc(dout)
        n, c, h, wd = dout.shape
        dx = torch.empty_like(dout)
        check(lib().saicv_row_scale(dtype_code(dout.dtype), ptr(dout), ptr(w), ptr(dx), n * h * wd, c, h * wd, stream()), 'row_scale')
        return dx, None


def sample_scale(x, w):
    return SampleScaleFn.apply(x, w)


class BatchNorm2dFn(torch.autograd.Function):
    """nn.BatchNorm2d on an activation that is not a convolution output (reference van.py:176,178,260; convformer.py:34-35,
    143,149): statistics pass -> the finalize kernel of the fused blocks (running statistics, num_batches_tracked) -> apply;
    backward = the fused blocks' BatchNorm backward without a ReLU gate."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn):
        require_gpu(x, gamma)
        x = _nhwc(x)
        dt = x.dtype
        n, c, h, w = x.shape
        M = n * h * w
        L, st, dev = lib(), stream(), x.device
        scale = torch.empty(c, dtype=torch.float32, device=dev)
        shift = torch.empty(c, dtype=torch.float32, device=dev)
        training = bn.training or not bn.track_running_stats
        if training:
            run = _RunningStats(bn, bn.training and bn.track_running_stats)
            stats = torch.zeros((2, c), dtype=torch.float32, device=dev)
            check(L.saicv_bn_stats(dtype_code(dt), ptr(x), M, c, ptr(stats[0]), ptr(stats[1]), st), 'bn_stats')
            mean = torch.empty(c, dtype=torch.float32, device=dev)
            invstd = torch.empty(c, dtype=torch.float32, device=dev)
            run.finalize(stats[0], stats[1], 1, c, M, gamma, beta, mean, invstd, scale, shift, st)
        else:
            check(L.saicv_bn_eval_coeffs(c, ptr(gamma), ptr(beta), ptr(bn.running_mean), ptr(bn.running_var), float(bn.eps),
                                         ptr(scale), ptr(shift), st), 'bn_eval_coeffs')
        z = torch.empty_like(x)
        check(L.saicv_bn_act_fwd(dtype_code(dt), ptr(x), 0, ptr(z), ptr(scale), ptr(shift), M, c, 0, 0, st), 'bn_act_fwd')
        if training:
            ctx.save_for_backward(x, gamma, mean, invstd)
        else:
            # frozen statistics: dx needs only scale; the affine parameters still get gradients (torch does the same in eval mode):
            # dgamma = sum dz * (x - running_mean) * rsqrt(running_var + eps), dbeta = sum dz -- keep x only when one is asked for
            need_affine = bool(gamma.requires_grad or (beta is not None and beta.requires_grad))
            if need_affine:
                rinv = torch.rsqrt(bn.running_var.detach().float() + float(bn.eps))
                ctx.save_for_backward(x, bn.running_mean.detach().float().clone(), rinv, scale)
            else:
                ctx.save_for_backward(None, None, None, scale)
        ctx.training = training
        return z

    @staticmethod
    def backward(ctx, dz):
        x, gamma, mean, invstd = ctx.saved_tensors
        L, st = lib(), stream()
        dz = _nhwc(dz)
        n, c, h, w = dz.shape
        M = n * h * w
        if not ctx.training:
            # frozen statistics: dx = scale * dz (invstd holds scale here); with x saved also the affine gradients
            dt = dz.dtype
            dx = torch.empty_like(dz)
            if x is None:
                check(L.saicv_channel_scale_add_bwd(dtype_code(dt), ptr(dz), 0, ptr(invstd), ptr(dx), 0, M, c, st), 'bn_eval_bwd')
                return dx, None, None, None
            rmean, rinv, scale = gamma, mean, invstd            # the eval-mode save order: (x, running_mean, rsqrt(var + eps), scale)
            if dz.dtype != x.dtype:
                dz = dz.to(x.dtype)
                dx = torch.empty_like(dz)
            sums = torch.zeros((3, c), dtype=torch.float32, device=dz.device)      # sum dz | sum dz^2 (unused) | sum dz * x
            check(L.saicv_bn_stats(dtype_code(dz.dtype), ptr(dz), M, c, ptr(sums[0]), ptr(sums[1]), st), 'bn_eval_bwd_sum')
            check(L.saicv_channel_scale_add_bwd(dtype_code(dz.dtype), ptr(dz), ptr(x), ptr(scale), ptr(dx), ptr(sums[2]), M, c, st),
                  'bn_eval_bwd')
            dbeta = sums[0]
            dgamma = rinv * (sums[2] - rmean * dbeta)
            return dx, dgamma, dbeta.clone(), None
        dt = x.dtype
        if dz.dtype != dt:
            dz = dz.to(dt)
        dx = torch.empty_like(x)
        dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
        ws = torch.empty(L.saicv_bn_bwd_ws_floats(M, c, dtype_code(dt)), dtype=torch.float32, device=x.device)
        check(L.saicv_bn_act_bwd(dtype_code(dt), ptr(dz), 0, 0, ptr(x), ptr(gamma), ptr(mean), ptr(invstd), ptr(dx), 0, ptr(dgamma),
                                 ptr(dbeta), M, c, 0, 0, ptr(ws), st), 'bn_act_bwd')
        return dx, dgamma, dbeta, None


def batch_norm2d(x, bn):
    """bn: the nn.BatchNorm2d holding the parameters and running statistics"""
    return BatchNorm2dFn.apply(x, bn.weight, bn.bias, bn)


class GroupNormFn(torch.autograd.Function):
    """nn.GroupNorm (+ the ReLU behind it) on an NHWC activation in the compute dtype, fp32 arithmetic (csrc/groupnorm.hip): the
    normalisation of the FCOS head towers (reference detection/models/head.py:101-124).  Two streaming passes each way."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, relu):
        require_gpu(x)
        x = _nhwc(x)
        n, c, h, w = x.shape
        dev = x.device
        mean_rstd = torch.empty((2, n, groups), dtype=torch.float32, device=dev)
        ab = torch.empty((2, n, c), dtype=torch.float32, device=dev)
        ws = torch.empty(lib().saicv_groupnorm_ws_floats(n, c), dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        check(lib().saicv_groupnorm_fwd(dtype_code(x.dtype), ptr(x), ptr(weight), ptr(bias), ptr(y), ptr(mean_rstd), ptr(ab), ptr(ws),
                                        n, h * w, c, groups, float(eps), int(relu), stream()), 'groupnorm_fwd')
        ctx.save_for_backward(x, weight, bias, mean_rstd, ab)
        ctx.cfg = (groups, bool(relu))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mean_rstd, ab = ctx.saved_tensors
        groups, relu = ctx.cfg
        n, c, h, w = x.shape
        dy = _nhwc(dy, x.dtype)
        dev = x.device
        dx = torch.empty_like(x)
        want_w = weight is not None and ctx.needs_input_grad[1]
        want_b = bias is not None and ctx.needs_input_grad[2]
        gw = _arena_grad(weight) if want_w else None
        gb = _arena_grad(bias) if want_b else None
        dgamma = gw if gw is not None else (torch.zeros(c, dtype=torch.float32, device=dev) if want_w else None)
        dbeta = gb if gb is not None else (torch.zeros(c, dtype=torch.float32, device=dev) if want_b else None)
        ws = torch.empty(lib().saicv_groupnorm_ws_floats(n, c), dtype=torch.float32, device=dev)
        check(lib().saicv_groupnorm_bwd(dtype_code(x.dtype), ptr(dy), ptr(x), ptr(weight), ptr(mean_rstd), ptr(ab), ptr(dx), ptr(dgamma),
                                        ptr(dbeta), ptr(ws), n, h * w, c, groups, int(relu), stream()), 'groupnorm_bwd')
        return (dx, dgamma if (want_w and gw is None) else None, dbeta if (want_b and gb is None) else None, None, None, None)


def group_norm(x, gn, relu=False):
    """gn: the nn.GroupNorm holding the parameters; under autocast the activation is normalised in the autocast dtype's storage
    with fp32 arithmetic (the reference's autocast runs group_norm in fp32 and the next convolution casts its input back)"""
    if torch.is_autocast_enabled('cuda') and x.is_floating_point() and x.dtype != compute_dtype():
        x = x.to(compute_dtype())
    return GroupNormFn.apply(x, gn.weight, gn.bias, gn.num_groups, gn.eps, relu)


class LinearFn(torch.autograd.Function):
    """y = x @ W^T + b on the implicit-GEMM kernel (1x1 geometry).  nn.Linear of resnet.py:204."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_f32):
        require_gpu(x, weight)
        if x.dim() != 2:
            raise ValueError('LinearFn expects a 2-d input')
        x = x.contiguous()
        dt = x.dtype
        b, ci = x.shape
        o = weight.shape[0]
        e = _lib.epc(dt)
        if ci % e:
            raise ValueError(f'linear: in_features={ci} must be a multiple of {e}')
        op = ((o + e - 1) // e) * e              # out_features padded to the 16-byte chunk
        wf, wd = packed_weight(weight, dt, ci, ctx.needs_input_grad[0], op)
        d = _desc(b, 1, 1, ci, op, 1, 1, 1, 0, dt)
        odt = torch.float32 if (out_f32 or dt == torch.float32) else dt
        y = torch.empty((b, op), dtype=odt, device=x.device)
        bp = bias
        if bias is not None and op != o:
            bp = torch.zeros(op, dtype=torch.float32, device=x.device)
            bp[:o] = bias.detach()
        t0 = KernelTimer.begin('linear_head')
        check(lib().saicv_conv2d_fwd(ctypes.byref(d), ptr(x), ptr(wf), ptr(bp), ptr(y),
                                     int(odt == torch.float32), 0, 0, stream()), 'linear_fwd')
        KernelTimer.end(t0, 'linear_head', 2.0 * b * ci * o, 0)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (d, wd, bias is not None, o, op)
        return y if op == o else y[:, :o]

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        d, wd, has_bias, o, op = ctx.cfg
        dt = x.dtype
        L = lib()
        st = stream()
        if op != o:
            dyp = torch.zeros((dy.shape[0], op), dtype=dt, device=dy.device)
            dyp[:, :o] = dy
            dy = dyp
        else:
            dy = dy.contiguous()
            if dy.dtype != dt:
                dy = dy.to(dt)
        b, ci = x.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if wd is None:
                _, wd = packed_weight(weight, dt, ci, True, op)
            dx = torch.empty((b, ci), dtype=dt, device=x.device)
            check(L.saicv_conv2d_dgrad(ctypes.byref(d), ptr(dy), ptr(wd), ptr(dx), st), 'linear_dgrad')
        if ctx.needs_input_grad[1]:
            dw = torch.zeros((op, ci), dtype=torch.float32, device=x.device)
            check(L.saicv_conv2d_wgrad(ctypes.byref(d), ptr(dy), ptr(x), ptr(dw), st), 'linear_wgrad')
            dw = dw[:o]
        if has_bias and ctx.needs_input_grad[2]:
            db = torch.zeros(op, dtype=torch.float32, device=x.device)
            check(L.saicv_colsum(dtype_code(dt), ptr(dy), b, op, ptr(db), st), 'colsum')
            db = db[:o]
        return dx, dw, db, None


def linear(x, weight, bias=None, out_f32=False):
    return LinearFn.apply(x, weight, bias, out_f32)


# ------------------------------------------------------------------------------ pooling
class MaxPoolFn(torch.autograd.Function):
    """nn.MaxPool2d(k, s, p) on NHWC (reference resnet.py:184)."""

    @staticmethod
    def forward(ctx, x, k, stride, pad):
        require_gpu(x)
        x = _nhwc(x)
        n, c, h, w = x.shape
        oh = (h + 2 * pad - k) // stride + 1
        ow = (w + 2 * pad - k) // stride + 1
        out = _empty_nhwc(n, c, oh, ow, x.dtype, x.device)
        idx = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=x.device)
        check(lib().saicv_maxpool_fwd(dtype_code(x.dtype), ptr(x), ptr(out), ptr(idx), n, h, w, c, oh, ow, k,
                                      stride, pad, stream()), 'maxpool_fwd')
        ctx.save_for_backward(idx)
        ctx.cfg = (n, c, h, w, oh, ow, k, stride, pad)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        n, c, h, w, oh, ow, k, stride, pad = ctx.cfg
        dout = _nhwc(dout)
        dx = _empty_nhwc(n, c, h, w, dout.dtype, dout.device)
        check(lib().saicv_maxpool_bwd(dtype_code(dout.dtype), ptr(dout), ptr(idx), ptr(dx), n, h, w, c, oh, ow,
                                      k, stride, pad, stream()), 'maxpool_bwd')
        return dx, None, None, None


def max_pool2d(x, k, stride, pad):
    return MaxPoolFn.apply(x, k, stride, pad)


class GlobalAvgPoolFn(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d((1,1)) + flatten -> [N, C] (reference resnet.py:203,243-244)."""

    @staticmethod
    def forward(ctx, x):
        require_gpu(x)
        x = _nhwc(x)
        n, c, h, w = x.shape
        out = torch.empty((n, c), dtype=x.dtype, device=x.device)
        check(lib().saicv_avgpool_fwd(dtype_code(x.dtype), ptr(x), ptr(out), n, h * w, c, stream()), 'avgpool_fwd')
        ctx.cfg = (n, c, h, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        n, c, h, w = ctx.cfg
        dout = dout.contiguous()
        dx = _empty_nhwc(n, c, h, w, dout.dtype, dout.device)
        check(lib().saicv_avgpool_bwd(dtype_code(dout.dtype), ptr(dout), ptr(dx), n, h * w, c, stream()),
              'avgpool_bwd')
        return dx


def global_avg_pool(x):
    return GlobalAvgPoolFn.apply(x)


# ------------------------------------------------------------------------------ losses
class SoftmaxCEFn(torch.autograd.Function):
    """mean softmax cross-entropy on fp32 logits; hard (int64) or soft (fp32 [B,C]) labels.

    Reference SimpleAICV/classification/losses.py:21-28 (CELoss), :86-91 (OneHotLabelCELoss)."""

    @staticmethod
    def forward(ctx, logits, label, soft):
        require_gpu(logits, label)
        logits = logits.float().contiguous()
        b, c = logits.shape
        if soft:
            label = label.float().contiguous()
        else:
            label = label.long().contiguous()
        dev = logits.device
        row = torch.empty(b, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad[0]
        dlog = torch.empty((b, c), dtype=torch.float32, device=dev) if need else None
        check(lib().saicv_softmax_ce_fwd(ptr(logits), ptr(label), int(soft), b, c, ptr(row), ptr(loss), ptr(dlog),
                                         stream()), 'softmax_ce_fwd')
        if need:
            ctx.save_for_backward(dlog)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (dlog,) = ctx.saved_tensors
        gout = gout.float().contiguous()
        out = torch.empty_like(dlog)
        check(lib().saicv_scale_by_scalar(_lib.F32, ptr(dlog), ptr(gout), ptr(out), dlog.numel(), stream()),
              'scale_by_scalar')
        return out, None, None


def softmax_cross_entropy(logits, label, soft=False):
    return SoftmaxCEFn.apply(logits, label, soft)


class _LastCall:
    """The last call of an entry whose result several losses over one prediction share: weak references to the two operands, their
    versions, the grad mode and the entry's other arguments.  Only one call is remembered, and the entry dies with either operand,
    so it never outlives the prediction it describes."""

    def __init__(self):
        self.entry = None

    def _forget(self, dead):
        e = self.entry
        if e is not None and (e[0] is dead or e[1] is dead):
            self.entry = None

    @staticmethod
    def _key(a, b, extras):
        return (a._version, b._version, torch.is_grad_enabled(), a.requires_grad) + extras

    def get(self, a, b, *extras):
        e = self.entry
        if e is not None and e[0]() is a and e[1]() is b and e[2] == self._key(a, b, extras):
            return e[3]
        return None

    def put(self, a, b, result, *extras):
        self.entry = (weakref.ref(a, self._forget), weakref.ref(b, self._forget), self._key(a, b, extras), result)
        return result


def _class_rows(logits, label, who):
    """[B, C, H, W] logits (NHWC memory is used as it is) or their [rows, C] view, on a 16-byte boundary, and the labels as one fp32
    row -> (x, lab, rows, c)"""
    if logits.dim() == 4:
        x = _nhwc(logits)
        rows = x.shape[0] * x.shape[2] * x.shape[3]
    elif logits.dim() == 2:
        x = logits.contiguous()
        rows = x.shape[0]
    else:
        raise ValueError(f'{who} expects [B, C, H, W] logits or their [rows, C] NHWC view')
    if x.data_ptr() % 16:
        x = x.clone(memory_format=torch.preserve_format)
    lab = label.reshape(-1).float().contiguous()
    if lab.numel() != rows:
        raise ValueError(f'{who}: {rows} pixels but {lab.numel()} labels')
    return x, lab, rows, x.shape[1]


class PixelSoftmaxCEFn(torch.autograd.Function):
    """The reference's semantic-segmentation CELoss (SimpleAICV/semantic_segmentation/losses.py:13-43) as one kernel each way
    (csrc/semseg.hip): softmax over the class axis, clamp to [1e-4, 1 - 1e-4], -log at the labelled class, mean over the pixels.
    The logits stay in their dtype (bf16 or fp32) and NHWC layout -- no fp32 copy, no permute, no one-hot; the forward keeps the
    per-pixel log-sum-exp, the backward reads the logits once and writes the gradient once.  No host read: the step can be captured."""

    @staticmethod
    def forward(ctx, logits, label):
        require_gpu(logits, label)
        logits, label, rows, c = _class_rows(logits, label, 'pixel_softmax_ce')
        L, dev = lib(), logits.device
        lse = torch.empty(rows, dtype=torch.float32, device=dev)
        partial = torch.empty(L.saicv_pixel_softmax_ce_ws_floats(rows), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        nbytes = rows * c * logits.element_size()
        t0 = KernelTimer.begin('pixel_ce')
        check(L.saicv_pixel_softmax_ce_fwd(dtype_code(logits.dtype), ptr(logits), ptr(label), rows, c, ptr(lse), ptr(partial),
                                           ptr(loss), stream()), 'pixel_softmax_ce_fwd')
        KernelTimer.end(t0, 'pixel_ce', 0, nbytes)
        ctx.save_for_backward(logits, label, lse)
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, label, lse = ctx.saved_tensors
        rows, c = lse.numel(), logits.shape[1]
        gout = gout.float().contiguous()
        dlog = torch.empty_like(logits)                      # preserves the NHWC strides of a 4-d prediction
        t0 = KernelTimer.begin('pixel_ce')
        check(lib().saicv_pixel_softmax_ce_bwd(dtype_code(logits.dtype), ptr(logits), ptr(label), ptr(lse), ptr(gout), rows, c,
                                               ptr(dlog), stream()), 'pixel_softmax_ce_bwd')
        KernelTimer.end(t0, 'pixel_ce', 0, 2 * rows * c * logits.element_size())
        return dlog, None


def pixel_softmax_ce(logits, label):
    """logits: [B, C, H, W] (any strides; NHWC memory is used as it is) or the [rows, C] NHWC view, bf16 or fp32, C <= 256;
    label: float (or integer) class ids, [B, H, W] or [rows].  -> scalar fp32 loss.
    A label outside [0, C) contributes neither loss nor gradient and still counts in the mean's denominator (the rule of
    softmax_cross_entropy); the reference's F.one_hot raises on such a label instead."""
    return PixelSoftmaxCEFn.apply(logits, label)


PIXEL_TERMS_FORMS = {'auto': 0, 'lane': 1, 'wave': 2}


class PixelClassTermsFn(torch.autograd.Function):
    """Everything the reference's parsing losses (SimpleAICV/human_parsing/losses.py:13-149: CELoss, MultiClassBCELoss, IoULoss,
    DiceLoss) read of the prediction, as one kernel each way (csrc/parsing.hip): -> fp32 [3] = (CE or multi-class BCE, IoU loss,
    Dice loss).  The logits stay in their dtype and NHWC layout; nothing per row is kept, the backward recomputes the row
    statistics from its one read of the logits and takes dL/dterms from device memory (no host read)."""

    @staticmethod
    def forward(ctx, logits, label, sigmoid, form):
        c = logits.shape[1]
        rows = logits.numel() // c
        L, dev = lib(), logits.device
        partial = torch.empty(L.saicv_pixel_class_terms_ws_floats(rows), dtype=torch.float32, device=dev)
        terms = torch.empty(3, dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('pixel_class_terms')
        check(L.saicv_pixel_class_terms_fwd(dtype_code(logits.dtype), ptr(logits), ptr(label), rows, c, sigmoid, form, ptr(partial),
                                            ptr(terms), stream()), 'pixel_class_terms_fwd')
        KernelTimer.end(t0, 'pixel_class_terms', 0, rows * c * logits.element_size())
        ctx.save_for_backward(logits, label)
        ctx.geom = (rows, c, sigmoid, form)
        return terms

    @staticmethod
    def backward(ctx, g):
        logits, label = ctx.saved_tensors
        rows, c, sigmoid, form = ctx.geom
        g = g.float().contiguous()
        dlog = torch.empty_like(logits)                      # preserves the NHWC strides of a 4-d prediction
        t0 = KernelTimer.begin('pixel_class_terms')
        check(lib().saicv_pixel_class_terms_bwd(dtype_code(logits.dtype), ptr(logits), ptr(label), ptr(g), rows, c, sigmoid, form,
                                                ptr(dlog), stream()), 'pixel_class_terms_bwd')
        KernelTimer.end(t0, 'pixel_class_terms', 0, 2 * rows * c * logits.element_size())
        return dlog, None, None, None


_pct_last = _LastCall()


def pixel_class_terms(logits, label, logit_type='softmax', form='auto'):
    """logits: [B, C, H, W] (any strides; NHWC memory is used as it is) or the [rows, C] NHWC view, bf16 or fp32, 2 <= C <= 256;
    label: float (or integer) class ids, [B, H, W] or [rows]; logit_type 'softmax' or 'sigmoid'.
    -> fp32 [3]: with a = softmax / sigmoid of the logits, q = clamp(a, 1e-4, 1 - 1e-4), I = q_t, S = sum_c q_c:
         [0] mean -log q_t (softmax: CELoss) or the mean binary cross-entropy over pixels and classes (sigmoid: MultiClassBCELoss),
         [1] mean 1 - I / max(S + 1 - I, 1e-4) (IoULoss),  [2] mean 1 - (2 I + 1e-4) / (S + 1 + 1e-4) (DiceLoss).
    A label outside [0, C) contributes to no term and no gradient and still counts in the means (the rule of pixel_softmax_ce).
    A second call with the same `logits` object at the same `_version`, the same `label` and logit type returns the SAME tensor:
    a criterion dict of several losses over one prediction costs one forward launch, and autograd adds the [3] gradients before
    the one backward launch.  Only the last call is remembered, through weak references to `logits` and `label` (see
    binary_seg_stats).  `form` picks the row mapping of csrc/parsing.hip ('lane', 'wave'; 'auto' = by class count)."""
    require_gpu(logits, label)
    if logit_type not in ('softmax', 'sigmoid'):
        raise ValueError(f"pixel_class_terms: logit_type is 'softmax' or 'sigmoid', got {logit_type!r}")
    terms = _pct_last.get(logits, label, logit_type, form)
    if terms is None:
        x, lab, _, _ = _class_rows(logits, label, 'pixel_class_terms')
        terms = _pct_last.put(logits, label, PixelClassTermsFn.apply(x, lab, int(logit_type == 'sigmoid'), PIXEL_TERMS_FORMS[form]),
                              logit_type, form)
    return terms


def _ctc_int(x, who):
    """lengths / targets -> int32, contiguous, on the device (a device-side cast: the reference passes trans_targets.float())"""
    if x.dtype == torch.bool or x.is_complex():
        raise ValueError(f'{who}: integer or floating tensor expected, got {x.dtype}')
    return x.to(torch.int32).contiguous()


def _ctc_rows(logits, who):
    if logits.dim() != 3:
        raise ValueError(f'{who} expects [T, B, C] logits, got {tuple(logits.shape)}')
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f'{who}: bf16 or fp32 logits, got {logits.dtype}')
    if logits.shape[2] > 1 and logits.stride(2) != 1:
        # no silent copy: at [64, 256, 12113] it would be the 0.4 - 0.8 GB this op exists to avoid
        raise ValueError(f'{who}: the class axis must have unit stride (t and b may have any), got strides {logits.stride()}; '
                         f'pass a view of a tensor whose last dimension is the classes')
    return logits


class CTCLossFn(torch.autograd.Function):
    """The reference's text-recognition CTCLoss (SimpleAICV/text_recognition/losses.py:21-46) in three launches forward and one
    backward (csrc/ctc.hip), on the [T, B, C] logits in their own dtype and strides: no fp32 copy, no log-softmax tensor.  Saved for
    the backward: the per-row log-sum-exp, the compact label log-probabilities and the per-class occupancies (T x B x (1 + S)
    floats each) -- not a dense gradient.  All sums are ordered; dL/dloss is read on the device."""

    @staticmethod
    def forward(ctx, logits, targets, input_lengths, target_lengths, blank, focal, gamma):
        L, dev = lib(), logits.device
        t, b, c = logits.shape
        s = targets.shape[1]
        ws = torch.empty(L.saicv_ctc_ws_floats(t, b, s), dtype=torch.float32, device=dev)
        nll = torch.empty(b, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('ctc_loss')
        check(L.saicv_ctc_loss_fwd(dtype_code(logits.dtype), ptr(logits), logits.stride(0), logits.stride(1), ptr(targets),
                                   ptr(input_lengths), ptr(target_lengths), t, b, s, c, blank, focal, gamma, ptr(ws), ptr(nll),
                                   ptr(loss), stream()), 'ctc_loss_fwd')
        KernelTimer.end(t0, 'ctc_loss', 0, t * b * c * logits.element_size())
        ctx.save_for_backward(logits, input_lengths, target_lengths, ws, nll)
        ctx.geom = (s, focal, gamma)
        ctx.mark_non_differentiable(nll)
        return loss, nll

    @staticmethod
    def backward(ctx, gout, _gnll):
        logits, input_lengths, target_lengths, ws, nll = ctx.saved_tensors
        s, focal, gamma = ctx.geom
        t, b, c = logits.shape
        gout = gout.float().contiguous()
        dlog = torch.empty_like(logits)                      # preserves the strides of the permuted [B, T, C] view
        if dlog.stride(2) != 1:
            dlog = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
        t0 = KernelTimer.begin('ctc_loss')
        check(lib().saicv_ctc_loss_bwd(dtype_code(logits.dtype), ptr(logits), logits.stride(0), logits.stride(1), ptr(dlog),
                                       dlog.stride(0), dlog.stride(1), ptr(input_lengths), ptr(target_lengths), ptr(ws), ptr(nll),
                                       ptr(gout), t, b, s, c, focal, gamma, stream()), 'ctc_loss_bwd')
        KernelTimer.end(t0, 'ctc_loss', 0, 2 * t * b * c * logits.element_size())
        return dlog, None, None, None, None, None, None


def ctc_loss(logits, targets, input_lengths, target_lengths, blank, focal_gamma=None):
    """logits [T, B, C] bf16 or fp32 with unit stride over C (any strides over T and B: the permuted view of the model's [B, T, C]
    output is used as it is); targets [B, S], input_lengths [B], target_lengths [B]: integer or floating device tensors.
    -> (loss, nll): loss = sum_b w_b nll_b / target_length_b / B with w_b = (1 - exp(-nll_b)) ** focal_gamma (1 when focal_gamma is
    None), the reference's CTCLoss; nll [B] fp32, detached.  zero_infinity: a sample whose labels do not fit its frames (or with a
    label outside [0, C) or equal to the blank) has nll 0, adds no loss and gets a zero gradient; entries of targets at or beyond
    a sample's target length are never used.  No host read: the call can be captured."""
    require_gpu(logits, targets, input_lengths, target_lengths)
    logits = _ctc_rows(logits, 'ctc_loss')
    t, b, c = logits.shape
    if targets.dim() != 2 or targets.shape[0] != b or input_lengths.numel() != b or target_lengths.numel() != b:
        raise ValueError(f'ctc_loss: batch {b}, targets {tuple(targets.shape)}, lengths {input_lengths.numel()} / '
                         f'{target_lengths.numel()}')
    if not 0 <= int(blank) < c:
        raise ValueError(f'ctc_loss: blank {blank} outside [0, {c})')
    focal = focal_gamma is not None
    if focal and not float(focal_gamma) >= 1.0:
        raise ValueError(f'ctc_loss: focal_gamma {focal_gamma}; at least 1 (the derivative holds (1 - p) ** (gamma - 1))')
    return CTCLossFn.apply(logits, _ctc_int(targets, 'ctc_loss'), _ctc_int(input_lengths.reshape(-1), 'ctc_loss'),
                           _ctc_int(target_lengths.reshape(-1), 'ctc_loss'), int(blank), int(focal),
                           float(focal_gamma) if focal else 0.0)


def ctc_greedy(logits, input_lengths=None):
    """logits [T, B, C] (as for ctc_loss) -> (index int32 [T, B], prob fp32 [T, B]): each frame's arg-max class (the lowest index
    among equals) and its softmax probability -- outputs.max(dim=2) and F.softmax(outputs, dim=2).max(dim=2) of the reference's
    validation loop without the softmax tensor.  Frames at or beyond input_lengths[b] get index -1 and probability 0."""
    require_gpu(logits)
    logits = _ctc_rows(logits.detach(), 'ctc_greedy')
    t, b, c = logits.shape
    lens = None
    if input_lengths is not None:
        require_gpu(input_lengths)
        if input_lengths.numel() != b:
            raise ValueError(f'ctc_greedy: batch {b} but {input_lengths.numel()} input lengths')
        lens = _ctc_int(input_lengths.reshape(-1), 'ctc_greedy')
    index = torch.empty((t, b), dtype=torch.int32, device=logits.device)
    prob = torch.empty((t, b), dtype=torch.float32, device=logits.device)
    t0 = KernelTimer.begin('ctc_greedy')
    check(lib().saicv_ctc_greedy(dtype_code(logits.dtype), ptr(logits), logits.stride(0), logits.stride(1),
                                 ptr(lens), t, b, c, ptr(index), ptr(prob), stream()), 'ctc_greedy')
    KernelTimer.end(t0, 'ctc_greedy', 0, t * b * c * logits.element_size())
    return index, prob


LSTM_WEIGHT_NAMES = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0',
                     'weight_ih_l0_reverse', 'weight_hh_l0_reverse', 'bias_ih_l0_reverse', 'bias_hh_l0_reverse')


def lstm_supports(input_size, hidden_size, dtype):
    """Whether ops.lstm runs this combination: bf16 or fp32, a hidden size that is a multiple of 32 in 32 .. 1024, an input size
    that is a multiple of the dtype's 16-byte chunk (8 bf16, 4 fp32)."""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    h, i = int(hidden_size), int(input_size)
    return 32 <= h <= 1024 and h % 32 == 0 and i >= 1 and i % _lib.epc(dtype) == 0


def _lstm_fragments(w, gates):
    """w [2, gates * H', K] (rows: gate-major) -> the MFMA B fragments in the order csrc/lstm.hip streams them,
    [2][H' / 16 slices][K chunks of 64 bytes][gates][64 lanes][16 bytes]: lane l of a fragment holds row 16 s + (l & 15), 16-byte
    piece l >> 4 of the chunk.  One copy; every load instruction of a wave then reads one contiguous KiB."""
    e = _lib.epc(w.dtype)
    two, rows, k = w.shape
    hs = rows // gates
    v = w.reshape(2, gates, hs // 16, 16, k // (4 * e), 4, e)            # [dir, g, slice, fr, chunk, fq, e]
    return v.permute(0, 2, 4, 1, 5, 3, 6).contiguous()                   # [dir, slice, chunk, g, fq, fr, e]


class LSTMFn(torch.autograd.Function):
    """One bidirectional nn.LSTM layer (batch_first, zero initial state).  Forward: the input projection of all frames and both
    directions as ONE GEMM with fp32 output (the stacked W_ih, b_ih + b_hh in the epilogue), then the recurrence of csrc/lstm.hip,
    which turns the pre-activations into the activated gates in place.  Saved: those gates [B T, 8H] fp32, c [B, T, 2H] fp32, y, x.
    Backward: the recurrence against the order writes dgates [B T, 8H] in the compute dtype; dx, dW_ih, dW_hh and the bias
    gradients are GEMMs / column sums over it on the implicit-GEMM kernels (fp32 weight gradients, ordered in deterministic mode)."""

    @staticmethod
    def forward(ctx, x, wih_f, whh_f, bih_f, bhh_f, wih_r, whh_r, bih_r, bhh_r):
        L, dev, dt = lib(), x.device, x.dtype
        b, t, i = x.shape
        h = whh_f.shape[1]
        x2 = x.reshape(b * t, i).contiguous()               # a row-strided view (padded out-features in front) is gathered here
        with torch.no_grad():
            wih = torch.cat([wih_f, wih_r])                                             # [8H, I]
            bias = torch.cat([bih_f + bhh_f, bih_r + bhh_r]).float()                    # [8H]
            whh = torch.stack([whh_f, whh_r]).to(dt)                                    # [2, 4H, H]
        wf, wd = packed_weight(wih, dt, i, ctx.needs_input_grad[0] and dt != torch.float32, 8 * h)
        d = _desc(b * t, 1, 1, i, 8 * h, 1, 1, 1, 0, dt)
        gates = torch.empty((b * t, 8 * h), dtype=torch.float32, device=dev)
        check(L.saicv_conv2d_fwd(ctypes.byref(d), ptr(x2), ptr(wf), ptr(bias), ptr(gates), 1, 0, 0, stream()), 'lstm input projection')
        y = torch.empty((b, t, 2 * h), dtype=dt, device=dev)
        c = torch.empty((b, t, 2 * h), dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('lstm_fwd')
        check(L.saicv_lstm_fwd(dtype_code(dt), ptr(gates), ptr(_lstm_fragments(whh, 4)), ptr(y), ptr(c), b, t, h, stream()),
              'lstm_fwd')
        KernelTimer.end(t0, 'lstm_fwd', 16.0 * b * t * h * h, 0)
        ctx.save_for_backward(x2, whh, gates, c, y)
        ctx.cfg = (d, wd, wih, (wih_f, wih_r), b, t, i, h)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, whh, gates, c, y = ctx.saved_tensors
        d, wd, wih, wih_dirs, b, t, i, h = ctx.cfg
        L, st, dev, dt = lib(), stream(), x2.device, x2.dtype
        dy = dy.contiguous()
        if dy.dtype != dt:
            dy = dy.to(dt)
        whh_t = _lstm_fragments(whh.transpose(1, 2), 1)                                 # [2, H, 4H] in fragment order: once per call
        dgates = torch.empty((b * t, 8 * h), dtype=dt, device=dev)
        t0 = KernelTimer.begin('lstm_bwd')
        check(L.saicv_lstm_bwd(dtype_code(dt), ptr(dy), ptr(gates), ptr(c), ptr(whh_t), ptr(dgates), b, t, h, st), 'lstm_bwd')
        KernelTimer.end(t0, 'lstm_bwd', 16.0 * b * t * h * h, 0)
        need = ctx.needs_input_grad
        dx = None
        if need[0] and dt == torch.float32:
            # fp32 (parity mode): one product per direction and their sum, as the reference's module forms dx -- sums of 4H terms
            # each, not one of 8H (the fp32 MFMA adds its K terms in one chain: at H = 512 the 8H chain alone used up the 4 x bound
            # of tests/lstm_common.py)
            d4 = _desc(b * t, 1, 1, i, 4 * h, 1, 1, 1, 0, dt)
            part = None
            for k, w_dir in enumerate(wih_dirs):
                _, wd_dir = packed_weight(w_dir, dt, i, True, 4 * h)
                dg = dgates[:, 4 * h * k:4 * h * (k + 1)].contiguous()
                dx = torch.empty((b * t, i), dtype=dt, device=dev)
                if part is None:
                    check(L.saicv_conv2d_dgrad(ctypes.byref(d4), ptr(dg), ptr(wd_dir), ptr(dx), st), 'lstm dx')
                else:
                    check(L.saicv_conv2d_dgrad_add(ctypes.byref(d4), ptr(dg), ptr(wd_dir), ptr(part), ptr(dx), st), 'lstm dx')
                part = dx
            dx = dx.view(b, t, i)
        elif need[0]:
            # bf16: ONE product over both directions' 8H columns, so that dx is rounded to bf16 once
            if wd is None:
                _, wd = packed_weight(wih, dt, i, True, 8 * h)
            dx = torch.empty((b * t, i), dtype=dt, device=dev)
            check(L.saicv_conv2d_dgrad(ctypes.byref(d), ptr(dgates), ptr(wd), ptr(dx), st), 'lstm dx')
            dx = dx.view(b, t, i)
        dwih_f = dwih_r = dwhh_f = dwhh_r = db_f = db_r = None
        if need[1] or need[5]:
            dwih = torch.zeros((8 * h, i), dtype=torch.float32, device=dev)
            check(L.saicv_conv2d_wgrad(ctypes.byref(d), ptr(dgates), ptr(x2), ptr(dwih), st), 'lstm dW_ih')
            dwih_f, dwih_r = dwih[:4 * h], dwih[4 * h:]
        if need[2] or need[6]:
            # h_{t-1} of each direction: y shifted one step in the direction's order, zero at its first step.  One GEMM over both
            # directions' columns; the two diagonal blocks of the [8H, 2H] product are the gradients
            hp = torch.zeros((b, t, 2 * h), dtype=dt, device=dev)
            if t > 1:
                hp[:, 1:, :h] = y[:, :-1, :h]
                hp[:, :-1, h:] = y[:, 1:, h:]
            d2 = _desc(b * t, 1, 1, 2 * h, 8 * h, 1, 1, 1, 0, dt)
            dwhh = torch.zeros((8 * h, 2 * h), dtype=torch.float32, device=dev)
            check(L.saicv_conv2d_wgrad(ctypes.byref(d2), ptr(dgates), ptr(hp), ptr(dwhh), st), 'lstm dW_hh')
            dwhh_f, dwhh_r = dwhh[:4 * h, :h], dwhh[4 * h:, h:]
        if any(need[k] for k in (3, 4, 7, 8)):
            db = torch.zeros(8 * h, dtype=torch.float32, device=dev)
            check(L.saicv_colsum(dtype_code(dt), ptr(dgates), b * t, 8 * h, ptr(db), st), 'lstm db')
            db_f, db_r = db[:4 * h], db[4 * h:]
        # (b_ih and b_hh enter as their sum: both get the column sums, each its own tensor)
        return (dx, dwih_f, dwhh_f, db_f, None if db_f is None else db_f.clone(), dwih_r, dwhh_r, db_r,
                None if db_r is None else db_r.clone())


def lstm(x, weights, bidirectional=True):
    """x [B, T, I] bf16 or fp32 (the last axis dense; rows may be strided) -> y [B, T, 2H]: torch.nn.LSTM(I, H, num_layers=1,
    batch_first=True, bidirectional=True) with zero initial state, no dropout, no projection.  weights: the module's tensors under
    its own names (a dict, e.g. dict(rnn.named_parameters())), or the eight of them in nn.LSTM's order.  See lstm_supports();
    anything else raises ValueError before a launch.  No host read: the call can be captured."""
    if not bidirectional:
        raise ValueError('lstm: only the bidirectional layer is built')
    if isinstance(weights, dict):
        missing = [n for n in LSTM_WEIGHT_NAMES if n not in weights]
        if missing:
            raise ValueError(f'lstm: weights lack {missing}')
        ws = [weights[n] for n in LSTM_WEIGHT_NAMES]
    else:
        ws = list(weights)
        if len(ws) != 8:
            raise ValueError(f'lstm: eight tensors expected (nn.LSTM order, both directions, both biases), got {len(ws)}')
    if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f'lstm expects [B, T, I] with B, T >= 1, got {tuple(x.shape)}')
    if x.shape[2] > 1 and x.stride(2) != 1:
        raise ValueError(f'lstm: the feature axis must have unit stride, got strides {x.stride()}')
    i, h = x.shape[2], ws[1].shape[1]
    if not lstm_supports(i, h, x.dtype):
        raise ValueError(f'lstm: input size {i}, hidden size {h}, {x.dtype} is not supported (lstm_supports)')
    for k in (0, 4):
        if tuple(ws[k].shape) != (4 * h, i) or tuple(ws[k + 1].shape) != (4 * h, h) or tuple(ws[k + 2].shape) != (4 * h,) \
                or tuple(ws[k + 3].shape) != (4 * h,):
            raise ValueError(f'lstm: weight shapes {[tuple(w.shape) for w in ws[k:k + 4]]} for input size {i}, hidden size {h}')
    require_gpu(x, *ws)
    return LSTMFn.apply(x, *ws)


class CpfeConvsFn(torch.autograd.Function):
    """x [N*H*W, Cin], W_all [(1 + 9 nb) P, Cin] -> the concatenated CPFE block output [N, (1 + nb) P, H, W] in `dtype`, NHWC
    memory: LinearFn's GEMM with fp32 output (Z), then the tap gather of csrc/semseg.hip.  One node for both, so that the
    backward's transposed gather hands dZ to the GEMM's gradient kernels in the compute dtype they read: between two nodes
    autograd would cast it to Z's fp32 and LinearFn back again, two passes over M x 28 P more."""

    @staticmethod
    def forward(ctx, x, w_all, n, h, w, p, dilations, dtype):
        nb = len(dilations)
        z = LinearFn.forward(ctx, x, w_all, None, True)       # saves (x, w_all) and its descriptor on ctx
        if z.shape != (n * h * w, (1 + 9 * nb) * p):
            raise ValueError('cpfe convs: W_all must hold (1 + 9 * branches) * P rows and x N*H*W rows')
        d = list(dilations) + [1] * (3 - nb)
        out = _empty_nhwc(n, (1 + nb) * p, h, w, dtype, z.device)
        t0 = KernelTimer.begin('cpfe_gather')
        check(lib().saicv_cpfe_gather_fwd(dtype_code(dtype), ptr(z), z.stride(0), ptr(out), n, h, w, p, nb, d[0], d[1], d[2], stream()),
              'cpfe_gather_fwd')
        KernelTimer.end(t0, 'cpfe_gather', 0, z.numel() * 4 + out.numel() * out.element_size())
        ctx.gather = (n, h, w, p, nb, d, dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        n, h, w, p, nb, d, dtype = ctx.gather
        dout = _nhwc(dout, dtype)
        dz = torch.empty((n * h * w, (1 + 9 * nb) * p), dtype=dtype, device=dout.device)
        t0 = KernelTimer.begin('cpfe_gather')
        check(lib().saicv_cpfe_gather_bwd(dtype_code(dtype), ptr(dout), ptr(dz), n, h, w, p, nb, d[0], d[1], d[2], stream()),
              'cpfe_gather_bwd')
        KernelTimer.end(t0, 'cpfe_gather', 0, (dz.numel() + dout.numel()) * dz.element_size())
        dx, dw, _, _ = LinearFn.backward(ctx, dz)
        return dx, dw, None, None, None, None, None, None


def cpfe_convs(x, w_1x1, w_dilated, dilations):
    """The four convolutions of a CPFE block (reference semantic_segmentation/models/pfan_semantic_segmentation.py:68-122) on one
    input: conv 1x1 and, per entry of `w_dilated`, conv 3x3 with dilation = padding = dilations[j], all Cin -> P without bias,
    concatenated along the channels -> [N, (1 + len(w_dilated)) * P, H, W] over NHWC memory, in the compute dtype.
    Because P << Cin, all of them are ONE GEMM Z = x . W_all^T over the stacked weight rows (fp32 output) plus a gather that sums
    each dilated branch's nine shifted taps.  W_all is assembled with torch ops, so every weight receives its own gradient."""
    require_gpu(x, w_1x1)
    if len(w_dilated) != len(dilations) or not 1 <= len(dilations) <= 3:
        raise ValueError('cpfe_convs: one dilation per dilated weight, 1 to 3 of them')
    dt = compute_dtype()
    x = _nhwc(x, dt)
    n, cin, h, w = x.shape
    p = w_1x1.shape[0]
    for wt in w_dilated:
        if tuple(wt.shape) != (p, cin, 3, 3):
            raise ValueError(f'cpfe_convs: a dilated weight is {tuple(wt.shape)}, expected {(p, cin, 3, 3)}')
    w_all = torch.cat([w_1x1.reshape(p, cin).float()] + [wt.float().permute(2, 3, 0, 1).reshape(9 * p, cin) for wt in w_dilated], dim=0)
    return CpfeConvsFn.apply(x.permute(0, 2, 3, 1).reshape(n * h * w, cin), w_all, n, h, w, p, tuple(int(d) for d in dilations), dt)


# ------------------------------------------------------------------------------ salient object detection (csrc/salient.hip)
C1_MIN_C, C1_MAX_C = 8, 64


def conv3x3_c1_supports(cin):
    """whether the one-channel head kernel takes `cin` input channels (a multiple of 8 from 8 to 64)"""
    return C1_MIN_C <= cin <= C1_MAX_C and cin % 8 == 0


class Conv3x3C1Fn(torch.autograd.Function):
    """nn.Conv2d(C, 1, kernel_size=3, padding=1, bias=True) + .float() + sigmoid, the prediction head of the salient-object PFAN
    (reference SimpleAICV/salient_object_detection/models/pfan_segmentation.py:254-300), as one streaming kernel each way
    (csrc/salient.hip): x stays NHWC in its dtype, the fp32 weight is read in place (no packing launch), the output is fp32
    [N, 1, H, W] and the logit is never rounded.  dw and db are ordered two-stage sums -- bit-reproducible in every mode -- and land
    in the arena when the engine offers the slots."""

    @staticmethod
    def forward(ctx, x, weight, bias, sigmoid):
        require_gpu(x, weight, bias)
        x = _nhwc(x)
        if x.data_ptr() % 16:
            x = x.clone(memory_format=torch.preserve_format)
        n, c, h, w = x.shape
        if tuple(weight.shape) != (1, c, 3, 3) or bias is None or bias.numel() != 1:
            raise ValueError(f'conv3x3_c1: weight {tuple(weight.shape)} / bias do not describe a 3x3 convolution {c} -> 1 with bias')
        if weight.dtype != torch.float32 or bias.dtype != torch.float32:
            raise ValueError('conv3x3_c1: weight and bias are the fp32 parameters')
        if not conv3x3_c1_supports(c):
            raise ValueError(f'conv3x3_c1: {c} input channels; the kernel takes a multiple of 8 from {C1_MIN_C} to {C1_MAX_C}')
        wuse = weight if weight.stride(2) == 3 * weight.stride(3) else weight.contiguous()
        out = torch.empty((n, 1, h, w), dtype=torch.float32, device=x.device)
        t0 = KernelTimer.begin('conv3x3_c1')
        check(lib().saicv_conv3x3_c1_fwd(dtype_code(x.dtype), ptr(x), ptr(wuse), wuse.stride(1), wuse.stride(3), ptr(bias), ptr(out),
                                         n, h, w, c, int(bool(sigmoid)), stream()), 'conv3x3_c1_fwd')
        KernelTimer.end(t0, 'conv3x3_c1', 2.0 * n * h * w * 9 * c, x.numel() * x.element_size() + out.numel() * 4)
        ctx.save_for_backward(x, weight, bias, out if sigmoid else None)
        ctx.sigmoid = bool(sigmoid)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, bias, out = ctx.saved_tensors
        n, c, h, w = x.shape
        dout = dout.float().contiguous()
        L, dev = lib(), x.device
        wuse = weight if weight.stride(2) == 3 * weight.stride(3) else weight.contiguous()
        want_x, want_w, want_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if want_x else None
        gw = _arena_grad(weight) if want_w and wuse is weight else None
        gb = _arena_grad(bias) if want_b else None
        # both sums leave one fold launch: they go straight into the arena only when every gradient that is wanted has a slot there
        direct = (want_w or want_b) and (not want_w or gw is not None) and (not want_b or gb is not None)
        if direct:
            dw, db = gw, gb
        else:
            dw = torch.empty_strided(wuse.shape, wuse.stride(), dtype=torch.float32, device=dev) if want_w else None
            db = torch.empty(bias.shape, dtype=torch.float32, device=dev) if want_b else None
        ws = torch.empty(L.saicv_conv3x3_c1_ws_floats(n, h, w, c), dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('conv3x3_c1')
        check(L.saicv_conv3x3_c1_bwd(dtype_code(x.dtype), ptr(x), ptr(wuse), wuse.stride(1), wuse.stride(3), ptr(out), ptr(dout),
                                     ptr(dx), ptr(dw), ptr(db), ptr(ws), n, h, w, c, int(ctx.sigmoid), int(direct), stream()),
              'conv3x3_c1_bwd')
        KernelTimer.end(t0, 'conv3x3_c1', 4.0 * n * h * w * 9 * c, (2 if want_x else 1) * x.numel() * x.element_size() + dout.numel() * 8)
        if direct:
            return dx, None, None, None
        return dx, dw, db, None


def conv3x3_c1(x, weight, bias, sigmoid=True):
    """x [N, C, H, W] (NHWC memory is used as it is; bf16 or fp32, C a multiple of 8 from 8 to 64), weight the fp32 parameter
    [1, C, 3, 3], bias fp32 [1] -> fp32 [N, 1, H, W]: sigmoid(conv(x) + b) or, with sigmoid=False, the logit.  Under autocast an
    fp32 activation is cast to the autocast dtype first, as torch.autocast casts a convolution's operands."""
    if torch.is_autocast_enabled('cuda') and x.is_floating_point() and x.dtype != compute_dtype():
        x = x.to(compute_dtype())
    return Conv3x3C1Fn.apply(x, weight, bias, sigmoid)


class BinarySegStatsFn(torch.autograd.Function):
    """prob, label fp32 [B, P] -> [B, 4] = (sum bce, sum ph, sum l, sum ph * l), ph = clamp(prob, 1e-4, 1 - 1e-4): everything the
    reference's BCELoss / BCEIouloss / BCEDiceLoss (SimpleAICV/salient_object_detection/losses.py:16-134) read of the full-resolution
    maps.  One read of both maps each way; the backward takes dL/dstats as a device tensor (no host read) and gives exactly 0
    outside the clamp, as torch.clamp's backward does."""

    @staticmethod
    def forward(ctx, prob, label):
        b, p = prob.shape
        L, dev = lib(), prob.device
        stats = torch.empty((b, 4), dtype=torch.float32, device=dev)
        partial = torch.empty(L.saicv_binary_seg_stats_ws_floats(b, p), dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('binary_seg_stats')
        check(L.saicv_binary_seg_stats_fwd(ptr(prob), ptr(label), b, p, ptr(partial), ptr(stats), stream()), 'binary_seg_stats_fwd')
        KernelTimer.end(t0, 'binary_seg_stats', 0, 8 * b * p)
        ctx.save_for_backward(prob, label)
        return stats

    @staticmethod
    def backward(ctx, g):
        prob, label = ctx.saved_tensors
        b, p = prob.shape
        g = g.float().contiguous()
        dprob = torch.empty_like(prob)
        t0 = KernelTimer.begin('binary_seg_stats')
        check(lib().saicv_binary_seg_stats_bwd(ptr(prob), ptr(label), ptr(g), b, p, ptr(dprob), stream()), 'binary_seg_stats_bwd')
        KernelTimer.end(t0, 'binary_seg_stats', 0, 12 * b * p)
        return dprob, None


_bss_last = _LastCall()


def binary_seg_stats(prob, label):
    """prob: fp32 contiguous probabilities [B, ...]; label: the soft mask with the same number of elements per sample, values in
    [0, 1] -> stats [B, 4] = per sample (sum bce, sum ph, sum l, sum ph * l) over ph = clamp(prob, 1e-4, 1 - 1e-4).
    A second call with the same `prob` object at the same `_version` and the same `label` returns the SAME stats tensor: a
    criterion dict of several losses over one prediction costs one forward launch, and autograd adds the [B, 4] gradients before
    the one backward launch.  Only the last call is remembered, and weakly: the entry refers to `prob` and `label` through weak
    references and goes when either of them does, so it never outlives the prediction it describes (the [B, 4] result itself is
    referenced: the losses keep only reductions of it alive, not the tensor)."""
    require_gpu(prob, label)
    if prob.dtype != torch.float32 or not prob.is_contiguous():
        raise ValueError('binary_seg_stats: prob must be fp32 and contiguous')
    stats = _bss_last.get(prob, label)
    if stats is not None:
        return stats
    b = prob.shape[0]
    p2 = prob.view(b, -1)
    l2 = label.reshape(b, -1)
    if l2.dtype != torch.float32 or not l2.is_contiguous():
        l2 = l2.float().contiguous()
    if l2.shape != p2.shape:
        raise ValueError(f'binary_seg_stats: prob has {p2.shape[1]} elements per sample, label {l2.shape[1]}')
    return _bss_last.put(prob, label, BinarySegStatsFn.apply(p2, l2))


# ------------------------------------------------------------------------------ human matting (csrc/matting.hip)
LAP_LEVELS = 5
LAP_MIN_SIDE = 32
_lap_default = [None]


def laplacian_gauss_table():
    """the 25 weights of the reference's build_gauss_kernel(size=5, sigma=1.0) (SimpleAICV/human_matting/losses.py:149-159) by the
    same numpy formula in float32: the SUM of the two axis Gaussians over the grid, normalised -- K[i, j] = (g_i + g_j) / S, not
    the product Gaussian.  -> a tuple of 25 floats, row-major"""
    if _lap_default[0] is None:
        import numpy as np
        size, sigma = 5, 1.0
        grid = np.float32(np.mgrid[0:size, 0:size].T)
        kernel = np.sum(np.exp(-((grid - size // 2) ** 2) / (2 * sigma ** 2)), axis=2)
        kernel /= np.sum(kernel)
        _lap_default[0] = tuple(float(v) for v in np.float32(kernel).reshape(-1))
    return _lap_default[0]


def _f32c(t):
    return t if t is None or (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _tri_layout(gp):
    """global_pred [B, 3, H, W] -> (fp32 tensor, (sb, sc, sp)): NCHW-contiguous and channels-last memory are read in place, anything
    else through a contiguous copy"""
    if gp.dim() != 4 or gp.shape[1] != 3:
        raise ValueError(f'global_pred must be [B, 3, H, W], got {tuple(gp.shape)}')
    if gp.dtype != torch.float32:
        gp = gp.float()
    if not (gp.is_contiguous() or gp.is_contiguous(memory_format=torch.channels_last)):
        gp = gp.contiguous()
    b, _, h, w = gp.shape
    sp = gp.stride(3) if w > 1 else (gp.stride(2) if h > 1 else 1)
    if h > 1 and w > 1 and gp.stride(2) != w * gp.stride(3):
        gp = gp.contiguous()
        sp = 1
    return gp, (gp.stride(0) if b > 1 else 3 * h * w, gp.stride(1), sp)


class TrimapStatsFn(torch.autograd.Function):
    """global_pred [B, 3, H, W] probabilities, trimap [B, H, W] -> [B, 2] = (sum of the 3-channel bce against the one-hot class, sum
    of the per-pixel IoU term): what GlobalTrimapCELoss and GloabelTrimapIouLoss (SimpleAICV/human_matting/losses.py:21-88) read of
    the maps.  One read each way; the backward takes dL/dstats on the device and is exactly 0 outside the clamp."""

    @staticmethod
    def forward(ctx, gp, trimap, smooth):
        gp, (sb, sc, sp) = _tri_layout(gp)
        b, p = gp.shape[0], gp.shape[2] * gp.shape[3]
        L, dev = lib(), gp.device
        stats = torch.empty((b, 2), dtype=torch.float32, device=dev)
        partial = torch.empty(L.saicv_matting_ws_floats(b, p), dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('trimap_stats')
        check(L.saicv_trimap_stats_fwd(ptr(gp), sb, sc, sp, ptr(trimap), b, p, float(smooth), ptr(partial), ptr(stats), stream()),
              'trimap_stats_fwd')
        KernelTimer.end(t0, 'trimap_stats', 0, 16 * b * p)
        ctx.save_for_backward(gp, trimap)
        ctx.layout, ctx.smooth = (sb, sc, sp), float(smooth)
        return stats

    @staticmethod
    def backward(ctx, g):
        gp, trimap = ctx.saved_tensors
        b, p = gp.shape[0], gp.shape[2] * gp.shape[3]
        sb, sc, sp = ctx.layout
        g = g.float().contiguous()
        dgp = torch.empty_like(gp)
        if dgp.stride() != gp.stride():
            raise RuntimeError('trimap_stats: the gradient did not take the layout of global_pred')
        t0 = KernelTimer.begin('trimap_stats')
        check(lib().saicv_trimap_stats_bwd(ptr(gp), sb, sc, sp, ptr(trimap), ptr(g), b, p, ctx.smooth, ptr(dgp), stream()),
              'trimap_stats_bwd')
        KernelTimer.end(t0, 'trimap_stats', 0, 28 * b * p)
        return dgp, None, None


def trimap_stats(global_pred, trimap, smooth=1e-4):
    """-> [B, 2] fp32: per sample (sum bce, sum of 1 - (ph_k + smooth) / (sum ph + 1 - ph_k + smooth)); class k of a trimap value:
    255 -> 2, else anything > 2 -> 1, else its integer part (the reference's order of rewrites)"""
    require_gpu(global_pred, trimap)
    trimap = _f32c(trimap)
    if trimap.numel() != global_pred.numel() // 3:
        raise ValueError(f'trimap_stats: global_pred {tuple(global_pred.shape)} and trimap {tuple(trimap.shape)} do not match')
    return TrimapStatsFn.apply(global_pred, trimap, smooth)


class AlphaL1Fn(torch.autograd.Function):
    """pred, alpha [B, P], trimap [B, P] or None -> [B, 2] = (sum sqrt(((ph - alpha) w)^2 + 1e-12), sum w), w = [trimap == 128] or 1:
    LocalAlphaLoss / FusionAlphaLoss (SimpleAICV/human_matting/losses.py:91-114, :183-203)"""

    @staticmethod
    def forward(ctx, pred, alpha, trimap):
        b, p = pred.shape
        L, dev = lib(), pred.device
        sums = torch.empty((b, 2), dtype=torch.float32, device=dev)
        partial = torch.empty(L.saicv_matting_ws_floats(b, p), dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('alpha_l1')
        check(L.saicv_alpha_l1_fwd(ptr(pred), ptr(alpha), ptr(trimap), b, p, ptr(partial), ptr(sums), stream()), 'alpha_l1_fwd')
        KernelTimer.end(t0, 'alpha_l1', 0, (8 if trimap is None else 12) * b * p)
        ctx.save_for_backward(pred, alpha, trimap)
        return sums

    @staticmethod
    def backward(ctx, g):
        pred, alpha, trimap = ctx.saved_tensors
        b, p = pred.shape
        g = g.float().contiguous()
        dpred = torch.empty_like(pred)
        t0 = KernelTimer.begin('alpha_l1')
        check(lib().saicv_alpha_l1_bwd(ptr(pred), ptr(alpha), ptr(trimap), ptr(g), b, p, ptr(dpred), stream()), 'alpha_l1_bwd')
        KernelTimer.end(t0, 'alpha_l1', 0, (12 if trimap is None else 16) * b * p)
        return dpred, None, None


def _maps(name, pred, *others):
    """pred [B, 1, H, W] or [B, H, W] and maps with the same number of pixels per sample -> fp32 contiguous [B, P] views"""
    require_gpu(pred, *others)
    b = pred.shape[0]
    out = [_f32c(pred).view(b, -1)]
    for t in others:
        t2 = None if t is None else _f32c(t).view(b, -1)
        if t2 is not None and t2.shape != out[0].shape:
            raise ValueError(f'{name}: pred has {out[0].shape[1]} pixels per sample, another map {t2.shape[1]}')
        out.append(t2)
    return out


def alpha_l1(pred, alpha, trimap=None):
    """-> [B, 2] fp32: per sample (sum sqrt(((clamp(pred) - alpha) w)^2 + 1e-12), sum w); w = [trimap == 128], or 1 without a
    trimap.  A pixel with w = 0 still adds sqrt(1e-12), as the reference's expression does."""
    return AlphaL1Fn.apply(*_maps('alpha_l1', pred, alpha, trimap))


class AlphaLossFn(torch.autograd.Function):
    """The alpha loss itself as one autograd node: sum_b sums[b, 0] / (sum_b sums[b, 1] + 1) with a trimap (LocalAlphaLoss), or
    / (B P) without (FusionAlphaLoss).  The same two kernels as AlphaL1Fn; the [B]-sized arithmetic around them is five small
    launches forward and two backward instead of the two dozen that autograd records for the same expression in torch ops (alone
    at batch 8, 1024^2 those made the fused LocalAlphaLoss launch-bound and slower than the composed one)."""

    @staticmethod
    def forward(ctx, pred, alpha, trimap):
        b, p = pred.shape
        L, dev = lib(), pred.device
        sums = torch.empty((b, 2), dtype=torch.float32, device=dev)
        partial = torch.empty(L.saicv_matting_ws_floats(b, p), dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('alpha_l1')
        check(L.saicv_alpha_l1_fwd(ptr(pred), ptr(alpha), ptr(trimap), b, p, ptr(partial), ptr(sums), stream()), 'alpha_l1_fwd')
        KernelTimer.end(t0, 'alpha_l1', 0, (8 if trimap is None else 12) * b * p)
        total = sums.sum(dim=0)
        den = total[1] + 1. if trimap is not None else torch.full((), float(b * p), dtype=torch.float32, device=dev)
        ctx.save_for_backward(pred, alpha, trimap, den)
        return total[0] / den

    @staticmethod
    def backward(ctx, g):
        pred, alpha, trimap, den = ctx.saved_tensors
        b, p = pred.shape
        gs = (g.float() / den).reshape(1, 1).expand(b, 2).contiguous()
        dpred = torch.empty_like(pred)
        t0 = KernelTimer.begin('alpha_l1')
        check(lib().saicv_alpha_l1_bwd(ptr(pred), ptr(alpha), ptr(trimap), ptr(gs), b, p, ptr(dpred), stream()), 'alpha_l1_bwd')
        KernelTimer.end(t0, 'alpha_l1', 0, (12 if trimap is None else 16) * b * p)
        return dpred, None, None


def alpha_loss(pred, alpha, trimap=None):
    """LocalAlphaLoss (trimap given: masked by [trimap == 128], denominator sum w + 1) / FusionAlphaLoss (no trimap: denominator
    the number of pixels) of the reference as a scalar; see alpha_l1 for the sums"""
    return AlphaLossFn.apply(*_maps('alpha_loss', pred, alpha, trimap))


class CompositionL1Fn(torch.autograd.Function):
    """pred [B, P]; fg, bg, image [B, 3 P] -> [B] = sum over pixels and channels of sqrt((ph fg + (1 - ph) bg - image)^2 + 1e-12):
    CompositionLoss (SimpleAICV/human_matting/losses.py:265-287); the gradient goes to pred only"""

    @staticmethod
    def forward(ctx, pred, fg, bg, image):
        b, p = pred.shape
        L, dev = lib(), pred.device
        sums = torch.empty((b,), dtype=torch.float32, device=dev)
        partial = torch.empty(L.saicv_matting_ws_floats(b, p), dtype=torch.float32, device=dev)
        t0 = KernelTimer.begin('composition_l1')
        check(L.saicv_composition_l1_fwd(ptr(pred), ptr(fg), ptr(bg), ptr(image), b, p, ptr(partial), ptr(sums), stream()),
              'composition_l1_fwd')
        KernelTimer.end(t0, 'composition_l1', 0, 40 * b * p)
        ctx.save_for_backward(pred, fg, bg, image)
        return sums

    @staticmethod
    def backward(ctx, g):
        pred, fg, bg, image = ctx.saved_tensors
        b, p = pred.shape
        g = g.float().contiguous()
        dpred = torch.empty_like(pred)
        t0 = KernelTimer.begin('composition_l1')
        check(lib().saicv_composition_l1_bwd(ptr(pred), ptr(fg), ptr(bg), ptr(image), ptr(g), b, p, ptr(dpred), stream()),
              'composition_l1_bwd')
        KernelTimer.end(t0, 'composition_l1', 0, 44 * b * p)
        return dpred, None, None, None


def composition_l1(pred, fg, bg, image):
    """pred [B, 1, H, W]; fg, bg, image [B, 3, H, W] -> [B] fp32"""
    require_gpu(pred, fg, bg, image)
    b = pred.shape[0]
    p2 = _f32c(pred).view(b, -1)
    three = [_f32c(t).view(b, -1) for t in (fg, bg, image)]
    if any(t.shape[1] != 3 * p2.shape[1] for t in three):
        raise ValueError('composition_l1: fg, bg and image must hold three channels of the prediction\'s size')
    return CompositionL1Fn.apply(p2, *three)


class LaplacianL1Fn(torch.autograd.Function):
    """pred, alpha [B, h, w], trimap or None -> sums [6, B]: sum |entry| of the six entries of ONE Laplacian pyramid of
    d0 = (clamp(pred) - alpha) * w.  The reference (SimpleAICV/human_matting/losses.py:117-180, :206-262) builds two pyramids and
    takes the l1 distance of their entries; the pyramid is linear, so that is the pyramid of the difference.  One launch per level
    each way (csrc/matting.hip); the five coarser maps (a third of a map) are what the backward keeps."""

    @staticmethod
    def forward(ctx, pred, alpha, trimap, table):
        b, h, w = pred.shape
        L, dev = lib(), pred.device
        tab = (ctypes.c_float * 25)(*table)
        sums = torch.empty((LAP_LEVELS + 1, b), dtype=torch.float32, device=dev)
        levels, cur = [], pred
        t0 = KernelTimer.begin('lap_level')
        for l in range(LAP_LEVELS):
            hl, wl = h >> l, w >> l
            nxt = torch.empty((b, hl // 2, wl // 2), dtype=torch.float32, device=dev)
            partial = torch.empty(L.saicv_lap_level_ws_floats(b, hl, wl), dtype=torch.float32, device=dev)
            top = l == LAP_LEVELS - 1
            check(L.saicv_lap_level_fwd(ptr(cur), ptr(alpha) if l == 0 else 0, ptr(trimap) if l == 0 else 0, int(l == 0), b, hl, wl,
                                        tab, ptr(nxt), ptr(partial), sums.data_ptr() + 4 * b * l,
                                        sums.data_ptr() + 4 * b * LAP_LEVELS if top else 0, stream()), 'lap_level_fwd')
            levels.append(nxt)
            cur = nxt
        KernelTimer.end(t0, 'lap_level', 50.0 * b * h * w * 4 / 3, (8 if trimap is None else 12) * b * h * w + 5 * b * h * w // 3 * 2)
        ctx.save_for_backward(pred, alpha, trimap, *levels)
        ctx.table = tuple(table)
        return sums

    @staticmethod
    def backward(ctx, g):
        pred, alpha, trimap, *levels = ctx.saved_tensors
        b, h, w = pred.shape
        L, dev = lib(), pred.device
        tab = (ctypes.c_float * 25)(*ctx.table)
        g = g.float().contiguous()
        maps = [pred] + list(levels)
        gnext = None
        t0 = KernelTimer.begin('lap_level')
        for l in range(LAP_LEVELS - 1, -1, -1):
            hl, wl = h >> l, w >> l
            top = l == LAP_LEVELS - 1
            gcur = torch.empty((b, hl, wl), dtype=torch.float32, device=dev)
            check(L.saicv_lap_level_bwd(ptr(maps[l]), ptr(alpha) if l == 0 else 0, ptr(trimap) if l == 0 else 0, int(l == 0), b, hl, wl,
                                        tab, ptr(gnext), ptr(maps[l + 1]) if top else 0, g.data_ptr() + 4 * b * l,
                                        g.data_ptr() + 4 * b * LAP_LEVELS if top else 0, ptr(gcur), stream()), 'lap_level_bwd')
            gnext = gcur
        KernelTimer.end(t0, 'lap_level', 100.0 * b * h * w * 4 / 3, (12 if trimap is None else 16) * b * h * w + 5 * b * h * w // 3 * 3)
        return gnext, None, None, None


def laplacian_sums(pred, alpha, trimap=None, weights=None):
    """-> sums [6, B] fp32 of the one-pyramid form; see laplacian_l1"""
    pred2, alpha2, trimap2 = (None if t is None else _f32c(t) for t in (pred, alpha, trimap))
    require_gpu(pred2, alpha2, trimap2)
    if pred2.dim() == 4:
        if pred2.shape[1] != 1:
            raise ValueError(f'laplacian_l1: pred must be [B, 1, H, W] or [B, H, W], got {tuple(pred.shape)}')
        pred2 = pred2.view(pred2.shape[0], pred2.shape[2], pred2.shape[3])
    b, h, w = pred2.shape
    if min(h, w) < LAP_MIN_SIDE:
        raise ValueError(f'laplacian_l1: a {h} x {w} map has no five pyramid levels; both sides must be at least {LAP_MIN_SIDE}')
    if tuple(alpha2.shape) != (b, h, w) or (trimap2 is not None and tuple(trimap2.shape) != (b, h, w)):
        raise ValueError(f'laplacian_l1: alpha / trimap must be [{b}, {h}, {w}]')
    table = laplacian_gauss_table() if weights is None else tuple(float(v) for v in torch.as_tensor(weights).reshape(-1).tolist())
    if len(table) != 25:
        raise ValueError('laplacian_l1: the weight table holds 25 values (5 x 5, row-major)')
    return LaplacianL1Fn.apply(pred2, alpha2, trimap2, table)


_lap_scales = {}


def _lap_scale(device, b, h, w):
    """1 / (elements of pyramid entry l) as a device tensor [6], made once per shape: the upload happens in the first (eager)
    iteration, so a step captured afterwards holds no host-to-device copy"""
    key = (device, b, h, w)
    if key not in _lap_scales:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('laplacian_l1: the first call at a new shape uploads a 6-element table and cannot be captured; '
                               'run one eager iteration first (config.step_graph_warmup >= 1)')
        _lap_scales[key] = torch.tensor([1. / (b * (h >> l) * (w >> l)) for l in range(LAP_LEVELS + 1)], dtype=torch.float32,
                                        device=device)
    return _lap_scales[key]


def laplacian_l1(pred, alpha, trimap=None, weights=None):
    """LocalLaplacianLoss (trimap given: both maps are masked by [trimap == 128]) / FusionLaplacianLoss (no trimap) of the
    reference: the sum over the six pyramid entries of their mean absolute difference.  pred [B, 1, H, W] probabilities (clamped
    to [1e-4, 1 - 1e-4] inside), alpha [B, H, W]; weights: the 25 values of the 5x5 filter (default: laplacian_gauss_table()).
    H, W >= 32 (ValueError otherwise, before any launch)."""
    sums = laplacian_sums(pred, alpha, trimap, weights)
    b, h, w = sums.shape[1], pred.shape[-2], pred.shape[-1]
    return (sums.sum(dim=1) * _lap_scale(sums.device, b, h, w)).sum()


class MattingFuseFn(torch.autograd.Function):
    """collaborative_matting (SimpleAICV/human_matting/models/pfan_matting.py:434-454): fused = local [argmax == 1] + [argmax == 2]
    over the first maximum of the three global probabilities; the gradient reaches local_pred where argmax == 1 and nothing else"""

    @staticmethod
    def forward(ctx, gp, local):
        gp, (sb, sc, sp) = _tri_layout(gp)
        b, p = gp.shape[0], gp.shape[2] * gp.shape[3]
        fused = torch.empty_like(local)
        t0 = KernelTimer.begin('matting_fuse')
        check(lib().saicv_matting_fuse_fwd(ptr(gp), sb, sc, sp, ptr(local), b, p, ptr(fused), stream()), 'matting_fuse_fwd')
        KernelTimer.end(t0, 'matting_fuse', 0, 20 * b * p)
        ctx.save_for_backward(gp)
        ctx.layout = (sb, sc, sp)
        return fused

    @staticmethod
    def backward(ctx, dfused):
        gp, = ctx.saved_tensors
        b, p = gp.shape[0], gp.shape[2] * gp.shape[3]
        sb, sc, sp = ctx.layout
        dfused = dfused.float().contiguous()
        dlocal = torch.empty_like(dfused)
        t0 = KernelTimer.begin('matting_fuse')
        check(lib().saicv_matting_fuse_bwd(ptr(gp), sb, sc, sp, ptr(dfused), b, p, ptr(dlocal), stream()), 'matting_fuse_bwd')
        KernelTimer.end(t0, 'matting_fuse', 0, 20 * b * p)
        return None, dlocal


def collaborative_matting(global_pred, local_pred):
    """global_pred [B, 3, H, W] (NCHW or channels-last memory), local_pred [B, 1, H, W] -> fused_pred [B, 1, H, W] fp32"""
    require_gpu(global_pred, local_pred)
    local = _f32c(local_pred)
    if local.dim() != 4 or local.shape[1] != 1 or local.numel() * 3 != global_pred.numel():
        raise ValueError(f'collaborative_matting: local_pred {tuple(local_pred.shape)} does not match global_pred {tuple(global_pred.shape)}')
    return MattingFuseFn.apply(global_pred, local)


# ------------------------------------------------------------------------------ SAM matting: grouped forms (csrc/matting.hip)
GROUP_MATTING_STATS = ('bce', 'iou', 'local_alpha', 'local_weight', 'fused_alpha', 'composition', 'intersection', 'union')


class GroupMattingStatsFn(torch.autograd.Function):
    """The raw sums of SAMMattingLoss (SimpleAICV/interactive_segmentation/losses_matting.py) for the M predictions of every sample
    against that sample's ONE set of targets: a target value is loaded once per pixel and serves all M masks; the backward writes
    every gradient element once and spends no read on a (b, m) row whose coefficients are all zero."""

    @staticmethod
    def forward(ctx, gp, lp, fp, alpha, trimap, image, fg, bg, thr):
        b, m = gp.shape[0], gp.shape[1]
        p = gp.shape[3] * gp.shape[4]
        L, dev = lib(), gp.device
        stats = torch.empty((b, m, len(GROUP_MATTING_STATS)), dtype=torch.float32, device=dev)
        partial = torch.empty(L.saicv_group_matting_ws_floats(b, m, p), dtype=torch.float32, device=dev)
        es = gp.element_size()
        t0 = KernelTimer.begin('group_matting_stats')
        check(L.saicv_group_matting_stats_fwd(dtype_code(gp.dtype), ptr(gp), ptr(lp), ptr(fp), ptr(alpha), ptr(trimap), ptr(image),
                                              ptr(fg), ptr(bg), b, m, p, float(thr), ptr(partial), ptr(stats), stream()),
              'group_matting_stats_fwd')
        KernelTimer.end(t0, 'group_matting_stats', 0, (44 + 5 * es * m) * b * p)
        ctx.save_for_backward(gp, lp, fp, alpha, trimap, image, fg, bg)
        return stats

    @staticmethod
    def backward(ctx, g):
        gp, lp, fp, alpha, trimap, image, fg, bg = ctx.saved_tensors
        b, m = gp.shape[0], gp.shape[1]
        p = gp.shape[3] * gp.shape[4]
        g = g.float().contiguous()
        dgp, dlp, dfp = torch.empty_like(gp), torch.empty_like(lp), torch.empty_like(fp)
        es = gp.element_size()
        t0 = KernelTimer.begin('group_matting_stats')
        check(lib().saicv_group_matting_stats_bwd(dtype_code(gp.dtype), ptr(gp), ptr(lp), ptr(fp), ptr(alpha), ptr(trimap),
                                                  ptr(image), ptr(fg), ptr(bg), ptr(g), b, m, p, ptr(dgp), ptr(dlp), ptr(dfp),
                                                  stream()), 'group_matting_stats_bwd')
        KernelTimer.end(t0, 'group_matting_stats', 0, (44 + 10 * es * m) * b * p)
        return dgp, dlp, dfp, None, None, None, None, None, None


def group_matting_stats(global_preds, local_preds, fused_preds, alpha, trimap, image, fg, bg, mask_threshold=0.5):
    """global_preds [B, M, 3, H, W], local_preds and fused_preds [B, M, 1, H, W] probabilities (fp32 or bf16, one dtype; clamped to
    [1e-4, 1 - 1e-4] in fp32 inside); alpha [B, 1, H, W], trimap [B, H, W], image, fg, bg [B, 3, H, W] -> fp32 [B, M, 8], the columns
    GROUP_MATTING_STATS: sum of the 3-channel bce against the one-hot trimap class, sum of the per-pixel IoU term (smooth 1e-4),
    sum sqrt(((local - alpha) w)^2 + 1e-12) and sum w (w = [trimap == 128]), sum sqrt((fused - alpha)^2 + 1e-12), the three-channel
    composition sum, and the counts of [fused > thr & alpha > thr] and of their union (whole numbers; no gradient, as sum w)."""
    require_gpu(global_preds, local_preds, fused_preds, alpha, trimap, image, fg, bg)
    if global_preds.dim() != 5 or global_preds.shape[2] != 3:
        raise ValueError(f'group_matting_stats: global_preds must be [B, M, 3, H, W], got {tuple(global_preds.shape)}')
    b, m, _, h, w = global_preds.shape
    dt = global_preds.dtype if global_preds.dtype in (torch.float32, torch.bfloat16) else torch.float32
    if local_preds.dtype != dt or fused_preds.dtype != dt:
        dt = torch.float32
    preds = []
    for name, t, c in (('global_preds', global_preds, 3), ('local_preds', local_preds, 1), ('fused_preds', fused_preds, 1)):
        if tuple(t.shape) != (b, m, c, h, w):
            raise ValueError(f'group_matting_stats: {name} must be [{b}, {m}, {c}, {h}, {w}], got {tuple(t.shape)}')
        preds.append(t.to(dt).contiguous())
    targets = []
    for name, t, c in (('alpha', alpha, 1), ('trimap', trimap, 1), ('image', image, 3), ('fg', fg, 3), ('bg', bg, 3)):
        if t.shape[0] != b or t.numel() != b * c * h * w:
            raise ValueError(f'group_matting_stats: {name} must hold [{b}, {c}, {h}, {w}] values, got {tuple(t.shape)}')
        targets.append(_f32c(t))
    return GroupMattingStatsFn.apply(*preds, *targets, float(mask_threshold))


class GroupLaplacianL1Fn(torch.autograd.Function):
    """LaplacianL1Fn for pred [B * M, h, w] against alpha / trimap [B, h, w]: only level 0 reads the targets, so the group is a
    parameter of that launch; the backward skips the pyramid pass of every row whose six coefficients are zero."""

    @staticmethod
    def forward(ctx, pred, alpha, trimap, table, group):
        r, h, w = pred.shape
        L, dev = lib(), pred.device
        tab = (ctypes.c_float * 25)(*table)
        sums = torch.empty((LAP_LEVELS + 1, r), dtype=torch.float32, device=dev)
        levels, cur = [], pred
        t0 = KernelTimer.begin('lap_level')
        for l in range(LAP_LEVELS):
            hl, wl = h >> l, w >> l
            nxt = torch.empty((r, hl // 2, wl // 2), dtype=torch.float32, device=dev)
            partial = torch.empty(L.saicv_lap_level_ws_floats(r, hl, wl), dtype=torch.float32, device=dev)
            top = l == LAP_LEVELS - 1
            if l == 0:
                check(L.saicv_lap_level0_group_fwd(ptr(cur), ptr(alpha), ptr(trimap), group, r, hl, wl, tab, ptr(nxt), ptr(partial),
                                                   sums.data_ptr(), stream()), 'lap_level0_group_fwd')
            else:
                check(L.saicv_lap_level_fwd(ptr(cur), 0, 0, 0, r, hl, wl, tab, ptr(nxt), ptr(partial), sums.data_ptr() + 4 * r * l,
                                            sums.data_ptr() + 4 * r * LAP_LEVELS if top else 0, stream()), 'lap_level_fwd')
            levels.append(nxt)
            cur = nxt
        KernelTimer.end(t0, 'lap_level', 50.0 * r * h * w * 4 / 3, 4 * r * h * w + (4 if trimap is None else 8) * r // group * h * w
                        + 5 * r * h * w // 3 * 2)
        ctx.save_for_backward(pred, alpha, trimap, *levels)
        ctx.table, ctx.group = tuple(table), group
        return sums

    @staticmethod
    def backward(ctx, g):
        pred, alpha, trimap, *levels = ctx.saved_tensors
        r, h, w = pred.shape
        L, dev = lib(), pred.device
        tab = (ctypes.c_float * 25)(*ctx.table)
        g = g.float().contiguous()
        maps = [pred] + list(levels)
        gnext = None
        t0 = KernelTimer.begin('lap_level')
        for l in range(LAP_LEVELS - 1, -1, -1):
            hl, wl = h >> l, w >> l
            top = l == LAP_LEVELS - 1
            gcur = torch.empty((r, hl, wl), dtype=torch.float32, device=dev)
            check(L.saicv_lap_level_group_bwd(ptr(maps[l]), ptr(alpha) if l == 0 else 0, ptr(trimap) if l == 0 else 0, int(l == 0),
                                              ctx.group, r, hl, wl, tab, ptr(gnext), ptr(maps[l + 1]) if top else 0,
                                              g.data_ptr() + 4 * r * l, g.data_ptr() + 4 * r * LAP_LEVELS if top else 0, ptr(g),
                                              LAP_LEVELS + 1, ptr(gcur), stream()), 'lap_level_group_bwd')
            gnext = gcur
        KernelTimer.end(t0, 'lap_level', 0, 4 * r * h * w)
        return gnext, None, None, None, None


def group_laplacian_sums(pred, alpha, trimap=None, weights=None):
    """laplacian_sums with M predictions per sample: pred [B, M, H, W] (or [B, M, 1, H, W]), alpha and trimap [B, H, W] (alpha also
    [B, 1, H, W]) -> sums [6, B * M] fp32, row b * M + m.  No expanded copy of a target is made."""
    pred2, alpha2, trimap2 = (None if t is None else _f32c(t) for t in (pred, alpha, trimap))
    require_gpu(pred2, alpha2, trimap2)
    if pred2.dim() == 5 and pred2.shape[2] == 1:
        pred2 = pred2.view(pred2.shape[0], pred2.shape[1], pred2.shape[3], pred2.shape[4])
    if pred2.dim() != 4:
        raise ValueError(f'group_laplacian_sums: pred must be [B, M, H, W] or [B, M, 1, H, W], got {tuple(pred.shape)}')
    b, m, h, w = pred2.shape
    if min(h, w) < LAP_MIN_SIDE:
        raise ValueError(f'group_laplacian_sums: a {h} x {w} map has no five pyramid levels; both sides must be at least '
                         f'{LAP_MIN_SIDE}')
    if alpha2.numel() != b * h * w or alpha2.shape[0] != b or (trimap2 is not None and tuple(trimap2.shape) != (b, h, w)):
        raise ValueError(f'group_laplacian_sums: alpha / trimap must be [{b}, {h}, {w}]')
    table = laplacian_gauss_table() if weights is None else tuple(float(v) for v in torch.as_tensor(weights).reshape(-1).tolist())
    if len(table) != 25:
        raise ValueError('group_laplacian_sums: the weight table holds 25 values (5 x 5, row-major)')
    return GroupLaplacianL1Fn.apply(pred2.view(b * m, h, w), alpha2.view(b, h, w), trimap2, table, m)


# ------------------------------------------------------------------------------ Muon: grouped Newton-Schulz (csrc/muon.hip)
MUON_TILE = 64
MUON_TAB = 13           # int32 per problem, the layout of csrc/muon.hip
MUON_COEFFS = (3.4445, -4.7750, 2.0315)


class MuonPlan:
    """Problem table and workspaces of one set of matrices: built once, every address fixed afterwards.
    `shapes`: (rows, cols) of each matrix in STORAGE order (row-major); `blocks`: first 1024-element arena block of each
    (engine.Muon), `ratios`: the lr factor of each.  Workspaces hold the operand in the wide orientation, padded with zeros to
    multiples of 64 (the padding is never written, so it stays zero)."""

    def __init__(self, shapes, device, blocks=None, ratios=None):
        import struct
        rows, xoff, aoff, sym, full, doff = [], 0, 0, 0, 0, 0
        self.items = []
        for k, (r, c) in enumerate(shapes):
            if r < 1 or c < 1:
                raise ValueError(f'muon: matrix {k} has shape {(r, c)}')
            tr = r > c
            m, n = (c, r) if tr else (r, c)
            mp, np_ = -(-m // MUON_TILE) * MUON_TILE, -(-n // MUON_TILE) * MUON_TILE
            ratio = struct.unpack('i', struct.pack('f', float(ratios[k]) if ratios is not None else 1.0))[0]
            rows.append([xoff, aoff, mp, np_, sym, full, blocks[k] if blocks is not None else 0, c, int(tr), ratio, m, n, doff])
            self.items.append((xoff, mp, np_, m, n, tr))
            tm = mp // MUON_TILE
            xoff, aoff, sym, full = xoff + mp * np_, aoff + mp * mp, sym + tm * (tm + 1) // 2, full + tm * (np_ // MUON_TILE)
            doff += mp
        if max(xoff, aoff) >= 2 ** 31:
            raise ValueError('muon: the packed workspaces exceed 2^31 elements')
        self.nprob, self.tiles_sym, self.tiles_full = len(rows), sym, full
        self.table = torch.tensor(rows if rows else [[0] * MUON_TAB], dtype=torch.int32).to(device)
        self.x = [torch.zeros(max(xoff, 8), dtype=torch.bfloat16, device=device) for _ in range(2)]
        self.a = torch.zeros(max(aoff, 8), dtype=torch.bfloat16, device=device)
        self.b = torch.zeros(max(aoff, 8), dtype=torch.bfloat16, device=device)
        # fp32 residuals of the diagonals of A and B (what their rounding to bf16 took away), one float per padded row
        self.da = torch.zeros(max(doff, 1), dtype=torch.float32, device=device)
        self.db = torch.zeros(max(doff, 1), dtype=torch.float32, device=device)
        self.partials = torch.zeros(max(len(rows), 1) * 32, dtype=torch.float32, device=device)

    def operand(self, k, buf=0):
        """[m][n] view of problem k's operand (wide orientation, without the padding) in workspace `buf`."""
        xoff, mp, np_, m, n, tr = self.items[k]
        return self.x[buf][xoff:xoff + mp * np_].view(mp, np_)[:m, :n]

    def run(self, steps, coeffs=MUON_COEFFS, normalize=True):
        """Newton-Schulz on the operands in workspace 0 -> index of the workspace that holds the result."""
        check(lib().saicv_muon_newton_schulz(ptr(self.x[0]), ptr(self.x[1]), ptr(self.a), ptr(self.b), ptr(self.da), ptr(self.db),
                                             ptr(self.table),
                                             self.nprob, self.tiles_sym, self.tiles_full, int(steps), float(coeffs[0]),
                                             float(coeffs[1]), float(coeffs[2]), int(bool(normalize)), ptr(self.partials),
                                             stream()), 'muon_newton_schulz')
        return int(steps) & 1


def muon_newton_schulz(tensors, steps=5, coeffs=MUON_COEFFS, normalize=True):
    """Newton-Schulz orthogonalisation (the reference's zeropower_via_newtonschulz5) of a LIST of 2-d tensors of mixed shapes
    in one set of grouped launches: X = bf16(t), transposed if rows > cols, X /= |X|_F + 1e-7 (if `normalize`), then `steps`
    times A = X X^T, B = b A + c A A, X = a X + B X.  -> list of bf16 tensors, each in its input's orientation."""
    tensors = list(tensors)
    if not tensors:
        return []
    require_gpu(*tensors)
    for t in tensors:
        if t.dim() != 2:
            raise ValueError(f'muon_newton_schulz takes 2-d tensors, got {tuple(t.shape)}')
    plan = MuonPlan([tuple(t.shape) for t in tensors], tensors[0].device)
    for k, t in enumerate(tensors):
        plan.operand(k).copy_(t.detach().t() if plan.items[k][5] else t.detach())
    buf = plan.run(steps, coeffs, normalize)
    out = []
    for k in range(len(tensors)):
        u = plan.operand(k, buf)
        out.append((u.t() if plan.items[k][5] else u).contiguous())
    return out


# ------------------------------------------------------------------------------ universal segmentation set loss (csrc/univseg.hip)
MATCHED_MASK_STATS = ('bce', 'intersection', 'pred_sum', 'target_sum')


def mask_pair_chunk():
    """Pixels per workgroup of the pair-sum and matched-statistics kernels: H * W is split into chunks of this length whose
    partial sums are added in chunk order."""
    return int(lib().saicv_univseg_chunk())


def _mask_offsets(offsets, b):
    host = [int(v) for v in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]
    if len(host) != b + 1 or host[0] != 0 or any(host[i + 1] < host[i] for i in range(b)):
        raise ValueError(f'offsets must be a non-decreasing table of {b + 1} entries starting at 0, got {host}')
    return host


def _mask_operands(mask_preds, targets, total):
    require_gpu(mask_preds, targets)
    if mask_preds.dim() != 4:
        raise ValueError(f'mask_preds must be [B, Q, H, W], got {tuple(mask_preds.shape)}')
    b, q, h, w = mask_preds.shape
    if mask_preds.dtype not in (torch.float32, torch.bfloat16):
        mask_preds = mask_preds.float()
    mask_preds = mask_preds.contiguous()
    targets = _f32c(targets)
    if tuple(targets.shape) != (total, h, w):
        raise ValueError(f'targets must be the packed [{total}, {h}, {w}] masks of the batch, got {tuple(targets.shape)}')
    return mask_preds, targets


def mask_pair_sums(mask_preds, targets, offsets):
    """mask_preds [B, Q, H, W] logits (bf16 or fp32), targets [sum T_i, H, W] in [0, 1] packed image after image, offsets the B + 1
    row bounds (a list or an int tensor; T_i = 0 is legal) -> (pos, neg, inter, pred_sum, target_sum), fp32:
    pos / neg / inter [Q, sum T_i] = sum_p softplus(-x) y, sum_p softplus(x)(1 - y), sum_p sigmoid(x) y, column offsets[i] + t
    paired with the queries of image i; pred_sum [B, Q] = sum_p sigmoid(x); target_sum [sum T_i] = sum_p y.  Ordered sums: the
    bits of an image's values depend on its own shapes alone, in every mode."""
    b = mask_preds.shape[0]
    host = _mask_offsets(offsets, b)
    total = host[-1]
    mask_preds, targets = _mask_operands(mask_preds, targets, total)
    q, p = mask_preds.shape[1], mask_preds.shape[2] * mask_preds.shape[3]
    L, dev = lib(), mask_preds.device
    off = torch.tensor(host, dtype=torch.int32).to(dev, non_blocking=True)
    sums = torch.empty(3 * q * total + b * q + total, dtype=torch.float32, device=dev)
    partial = torch.empty(L.saicv_univseg_pair_ws_floats(b, q, total, p), dtype=torch.float32, device=dev)
    tmax = max(host[i + 1] - host[i] for i in range(b))
    t0 = KernelTimer.begin('univseg_pair_sums')
    check(L.saicv_univseg_pair_sums(dtype_code(mask_preds.dtype), ptr(mask_preds), ptr(targets), ptr(off), b, q, total, tmax, p,
                                    ptr(partial), ptr(sums), stream()), 'univseg_pair_sums')
    KernelTimer.end(t0, 'univseg_pair_sums', 6.0 * q * total * p, mask_preds.element_size() * b * q * p + 4 * total * p)
    plane = q * total
    return (sums[:plane].view(q, total), sums[plane:2 * plane].view(q, total), sums[2 * plane:3 * plane].view(q, total),
            sums[3 * plane:3 * plane + b * q].view(b, q), sums[3 * plane + b * q:])


def mask_match_cost(mask_preds, class_preds, targets, offsets, labels, mask_cost=1.0, dice_cost=1.0, class_cost=1.0):
    """The cost matrices of Mask2FormerHungarianMatcher (universal_segmentation/segmentation_losses.py) for the whole batch, PACKED:
    fp32 [Q, sum T_i] on the device, columns offsets[i] .. offsets[i + 1) being image i's [Q, T_i] matrix
        mask_cost (P + N) / (H W) + dice_cost (1 - (2 S + 1) / (sum sigmoid + sum y + 1)) - class_cost softmax(class_preds)[q, label_t]
    clamped to +-1e10 with NaN -> 0.  class_preds [B, Q, C], labels the packed [sum T_i] class ids.  One copy to the host then serves
    every image's assignment."""
    b, q = mask_preds.shape[0], mask_preds.shape[1]
    host = _mask_offsets(offsets, b)
    pos, neg, inter, pred_sum, target_sum = mask_pair_sums(mask_preds, targets, host)
    dev = mask_preds.device
    counts = torch.tensor([host[i + 1] - host[i] for i in range(b)], dtype=torch.int64)
    image = torch.repeat_interleave(torch.arange(b, dtype=torch.int64), counts).to(dev, non_blocking=True)
    labels = labels.to(device=dev, dtype=torch.int64)
    hw = mask_preds.shape[2] * mask_preds.shape[3]
    probs = class_preds.float().softmax(dim=-1)
    cls = probs[image, :, labels].t()                                              # [Q, sum T]
    dice = 1 - (2 * inter + 1) / (pred_sum[image].t() + target_sum[None, :] + 1)
    cost = mask_cost * ((pos + neg) / hw) + dice_cost * dice - class_cost * cls
    return torch.nan_to_num(cost.clamp(min=-1e10, max=1e10), 0)


class MatchedMaskStatsFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, mask_preds, targets, rowx, rowy, rowmap):
        m = rowx.numel()
        p = mask_preds.shape[2] * mask_preds.shape[3]
        L, dev = lib(), mask_preds.device
        stats = torch.empty((m, 4), dtype=torch.float32, device=dev)
        if m:
            partial = torch.empty(L.saicv_univseg_matched_ws_floats(m, p), dtype=torch.float32, device=dev)
            t0 = KernelTimer.begin('univseg_matched')
            check(L.saicv_univseg_matched_fwd(dtype_code(mask_preds.dtype), ptr(mask_preds), ptr(targets), ptr(rowx), ptr(rowy), m, p,
                                              ptr(partial), ptr(stats), stream()), 'univseg_matched_fwd')
            KernelTimer.end(t0, 'univseg_matched', 0, (mask_preds.element_size() + 4) * m * p)
        ctx.save_for_backward(mask_preds, targets, rowy, rowmap)
        return stats

    @staticmethod
    def backward(ctx, g):
        mask_preds, targets, rowy, rowmap = ctx.saved_tensors
        b, q, h, w = mask_preds.shape
        g = g.float().contiguous()
        dpreds = torch.empty_like(mask_preds)
        t0 = KernelTimer.begin('univseg_matched')
        check(lib().saicv_univseg_matched_bwd(dtype_code(mask_preds.dtype), ptr(mask_preds), ptr(targets), ptr(rowmap), ptr(rowy),
                                              ptr(g), b * q, h * w, ptr(dpreds), stream()), 'univseg_matched_bwd')
        KernelTimer.end(t0, 'univseg_matched', 0, mask_preds.element_size() * (b * q + rowy.numel()) * h * w + 4 * rowy.numel() * h * w)
        return dpreds, None, None, None, None


def matched_mask_stats(mask_preds, targets, pair_b, pair_q, pair_t):
    """The pixel sums of the matched pairs of UniversalSegmentationLoss: pair m joins row (pair_b[m], pair_q[m]) of mask_preds
    [B, Q, H, W] (bf16 or fp32 logits) with row pair_t[m] of the packed targets [sum T_i, H, W] (pair_t indexes the PACKED rows:
    offsets[b] + t) -> fp32 [M, 4], the columns MATCHED_MASK_STATS: sum BCEWithLogits(x, y), sum sigmoid(x) y, sum sigmoid(x), sum y.
    Rows are read through the index tensors, no gather copy.  Differentiable in mask_preds: the backward writes the whole
    [B, Q, H, W] gradient in mask_preds' dtype, exact zeros in every unmatched row.  A (b, q) that occurs twice raises."""
    pb, pq, pt = (torch.as_tensor(t).reshape(-1).to('cpu', torch.int64) for t in (pair_b, pair_q, pair_t))
    if not (pb.numel() == pq.numel() == pt.numel()):
        raise ValueError('matched_mask_stats: pair_b, pair_q and pair_t must have one length')
    total = targets.shape[0]
    mask_preds, targets = _mask_operands(mask_preds, targets, total)
    b, q = mask_preds.shape[0], mask_preds.shape[1]
    m = pb.numel()
    if m and (int(pb.min()) < 0 or int(pb.max()) >= b or int(pq.min()) < 0 or int(pq.max()) >= q or int(pt.min()) < 0
              or int(pt.max()) >= total):
        raise ValueError('matched_mask_stats: a pair index is out of range')
    rows = pb * q + pq
    if torch.unique(rows).numel() != m:
        raise RuntimeError('matched_mask_stats: a (b, q) prediction row is matched twice; an assignment never does that')
    rowmap = torch.full((b * q, ), -1, dtype=torch.int32)
    rowmap[rows] = torch.arange(m, dtype=torch.int32)
    dev = mask_preds.device
    return MatchedMaskStatsFn.apply(mask_preds, targets, rows.to(torch.int32).to(dev, non_blocking=True),
                                    pt.to(torch.int32).to(dev, non_blocking=True), rowmap.to(dev, non_blocking=True))


# ------------------------------------------------------------------------------ universal matting (csrc/unimat.hip)
MATTING_PAIR_SUMS = ('ce_pos', 'ce_neg', 'intersection', 'local_l1', 'fused_l1')


def matting_pair_chunk():
    """Pixels per workgroup of the matting pair-sum kernel: H * W is split into chunks of this length, added in chunk order."""
    return int(lib().saicv_unimat_chunk())


def _matting_pred(t, channels, name):
    """[B, Q, channels, H, W] probabilities -> (fp32 tensor, (sb, sq, sc, sp)), read in place whenever the pixels of a (b, q, c) map
    lie one stride apart (the contiguous and the channels-last order both do); anything else through a contiguous copy"""
    if t.dim() != 5 or t.shape[2] != channels:
        raise ValueError(f'{name} must be [B, Q, {channels}, H, W], got {tuple(t.shape)}')
    if t.dtype != torch.float32:
        t = t.float()
    h, w = t.shape[3], t.shape[4]
    if (h > 1 and w > 1 and t.stride(3) != w * t.stride(4)) or any(s < 0 for s in t.stride()):
        t = t.contiguous()
    sp = t.stride(4) if w > 1 else (t.stride(3) if h > 1 else 1)
    return t, (t.stride(0), t.stride(1), t.stride(2), sp)


def matting_pair_sums(global_preds, local_preds, fused_preds, trimaps, alphas, offsets):
    """global_preds [B, Q, 3, H, W], local_preds and fused_preds [B, Q, 1, H, W] fp32 probabilities in any memory order whose
    pixel axis is one stride (read in place); trimaps, alphas [sum T_i, H, W] packed image after image; offsets the B + 1 row
    bounds (T_i = 0 is legal).  -> (planes [5, Q, sum T_i] in the order MATTING_PAIR_SUMS, global_sum [B, Q], weight_sum [sum T_i]),
    fp32; column offsets[i] + t of a plane is paired with the queries of image i.  Probabilities are clamped to [1e-4, 1 - 1e-4];
    class k of a trimap value as in trimap_stats; ordered sums, bit-reproducible."""
    require_gpu(global_preds, local_preds, fused_preds, trimaps, alphas)
    b, q = global_preds.shape[0], global_preds.shape[1]
    host = _mask_offsets(offsets, b)
    total = host[-1]
    gp, gs = _matting_pred(global_preds, 3, 'global_preds')
    lp, ls = _matting_pred(local_preds, 1, 'local_preds')
    fp, fs = _matting_pred(fused_preds, 1, 'fused_preds')
    h, w = gp.shape[3], gp.shape[4]
    if tuple(lp.shape) != (b, q, 1, h, w) or tuple(fp.shape) != (b, q, 1, h, w):
        raise ValueError(f'local_preds / fused_preds must be [{b}, {q}, 1, {h}, {w}]')
    trimaps, alphas = _f32c(trimaps), _f32c(alphas)
    if tuple(trimaps.shape) != (total, h, w) or tuple(alphas.shape) != (total, h, w):
        raise ValueError(f'trimaps and alphas must be the packed [{total}, {h}, {w}] maps of the batch')
    p = h * w
    L, dev = lib(), gp.device
    off = torch.tensor(host, dtype=torch.int32).to(dev, non_blocking=True)
    sums = torch.empty(5 * q * total + b * q + total, dtype=torch.float32, device=dev)
    partial = torch.empty(L.saicv_unimat_pair_ws_floats(b, q, total, p), dtype=torch.float32, device=dev)
    tmax = max(host[i + 1] - host[i] for i in range(b))
    t0 = KernelTimer.begin('unimat_pair_sums')
    check(L.saicv_unimat_pair_sums(ptr(gp), gs[0], gs[1], gs[2], gs[3], ptr(lp), ls[0], ls[1], ls[3], ptr(fp), fs[0], fs[1], fs[3],
                                   ptr(trimaps), ptr(alphas), ptr(off), b, q, total, tmax, p, ptr(partial), ptr(sums), stream()),
          'unimat_pair_sums')
    KernelTimer.end(t0, 'unimat_pair_sums', 0, 20 * b * q * p + 8 * total * p)
    plane = q * total
    return sums[:5 * plane].view(5, q, total), sums[5 * plane:5 * plane + b * q].view(b, q), sums[5 * plane + b * q:]


def matting_match_cost(global_preds, local_preds, fused_preds, class_preds, trimaps, alphas, offsets, labels, ce_cost=1.0,
                       iou_cost=1.0, local_cost=1.0, fusion_cost=1.0, class_cost=1.0):
    """The cost matrices of the universal-matting Mask2FormerHungarianMatcher (universal_segmentation/matting_losses.py) for the
    whole batch, PACKED: fp32 [Q, sum T_i] on the device, columns offsets[i] .. offsets[i + 1) being image i's [Q, T_i] matrix
        ce (Cpos + Cneg) / (3 P) + iou (1 - (I + 1e-4) / (G + P - I + 1e-4)) + local L / (W + 1) + fusion F / P
        - class softmax(class_preds)[q, label_t]
    clamped to +-1e10 with NaN -> 0 (the sums: matting_pair_sums).  One copy to the host then serves every image's assignment."""
    b = global_preds.shape[0]
    host = _mask_offsets(offsets, b)
    planes, gsum, wsum = matting_pair_sums(global_preds, local_preds, fused_preds, trimaps, alphas, host)
    dev = planes.device
    p = float(global_preds.shape[3] * global_preds.shape[4])
    counts = torch.tensor([host[i + 1] - host[i] for i in range(b)], dtype=torch.int64)
    image = torch.repeat_interleave(torch.arange(b, dtype=torch.int64), counts).to(dev, non_blocking=True)
    labels = labels.to(device=dev, dtype=torch.int64)
    cls = class_preds.float().softmax(dim=-1)[image, :, labels].t()                 # [Q, sum T]
    cpos, cneg, inter, lsum, fsum = planes
    iou = 1 - (inter + 1e-4) / (gsum[image].t() + p - inter + 1e-4)
    cost = (ce_cost * ((cpos + cneg) / (3 * p)) + iou_cost * iou + local_cost * (lsum / (wsum[None, :] + 1))
            + fusion_cost * (fsum / p) - class_cost * cls)
    return torch.nan_to_num(cost.clamp(min=-1e10, max=1e10), 0)


class MattingHeadFn(torch.autograd.Function):
    """channels-last logits [B, H, W, 3Q] and [B, H, W, Q] (bf16 or fp32) -> fp32 probabilities of the same shapes and the fused
    prediction, one pass each way"""

    @staticmethod
    def forward(ctx, gl, ll):
        b, h, w, q = ll.shape
        dev = gl.device
        g = torch.empty((b, h, w, 3 * q), dtype=torch.float32, device=dev)
        l = torch.empty((b, h, w, q), dtype=torch.float32, device=dev)
        f = torch.empty((b, h, w, q), dtype=torch.float32, device=dev)
        rows = b * h * w
        t0 = KernelTimer.begin('unimat_head')
        check(lib().saicv_unimat_head_fwd(dtype_code(gl.dtype), ptr(gl), ptr(ll), rows, q, ptr(g), ptr(l), ptr(f), stream()),
              'unimat_head_fwd')
        KernelTimer.end(t0, 'unimat_head', 0, (4 * gl.element_size() + 20) * rows * q)
        ctx.save_for_backward(g, l)
        ctx.dtype = gl.dtype
        return g, l, f

    @staticmethod
    def backward(ctx, dg, dl, df):
        g, l = ctx.saved_tensors
        b, h, w, q = l.shape
        dg, dl, df = (t.float().contiguous() for t in (dg, dl, df))
        dgl = torch.empty(g.shape, dtype=ctx.dtype, device=g.device)
        dll = torch.empty(l.shape, dtype=ctx.dtype, device=g.device)
        t0 = KernelTimer.begin('unimat_head')
        check(lib().saicv_unimat_head_bwd(dtype_code(ctx.dtype), ptr(g), ptr(l), ptr(dg), ptr(dl), ptr(df), b * h * w, q, ptr(dgl),
                                          ptr(dll), stream()), 'unimat_head_bwd')
        KernelTimer.end(t0, 'unimat_head', 0, (4 * dgl.element_size() + 36) * b * h * w * q)
        return dgl, dll


def matting_head(global_logits, local_logits):
    """The end of UniversalMatting.predict: global_logits [B, 3Q, H, W] (channel 3 q + c) and local_logits [B, Q, H, W], bf16 or
    fp32; channels-last memory is read in place, any other order through a copy.  -> (global_preds [B, Q, 3, H, W], local_preds
    [B, Q, 1, H, W], fused_preds [B, Q, 1, H, W]), fp32 VIEWS of channels-last memory: sigmoid, sigmoid, and
    local [argmax == 1] + [argmax == 2] with the argmax over the three fp32 probabilities (first maximum on ties, torch.max)."""
    require_gpu(global_logits, local_logits)
    if global_logits.dim() != 4 or local_logits.dim() != 4 or global_logits.shape[1] != 3 * local_logits.shape[1] \
            or global_logits.shape[0] != local_logits.shape[0] or global_logits.shape[2:] != local_logits.shape[2:]:
        raise ValueError(f'matting_head: global_logits {tuple(global_logits.shape)} must be [B, 3Q, H, W] for local_logits '
                         f'{tuple(local_logits.shape)} = [B, Q, H, W]')
    if global_logits.dtype != local_logits.dtype or global_logits.dtype not in (torch.float32, torch.bfloat16):
        global_logits, local_logits = global_logits.float(), local_logits.float()
    b, q, h, w = local_logits.shape
    g, l, f = MattingHeadFn.apply(global_logits.permute(0, 2, 3, 1).contiguous(), local_logits.permute(0, 2, 3, 1).contiguous())
    return (g.view(b, h, w, q, 3).permute(0, 3, 4, 1, 2), l.view(b, h, w, q, 1).permute(0, 3, 4, 1, 2),
            f.view(b, h, w, q, 1).permute(0, 3, 4, 1, 2))


class TakeRowsFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, pb, pq):
        ctx.save_for_backward(pb, pq)
        ctx.layout = (tuple(x.shape), tuple(x.stride()), x.dtype)
        return x[pb, pq].contiguous()

    @staticmethod
    def backward(ctx, g):
        pb, pq = ctx.saved_tensors
        shape, stride, dtype = ctx.layout
        dx = torch.empty_strided(shape, stride, dtype=dtype, device=g.device).zero_()
        dx[pb, pq] = g.to(dtype)
        return dx, None, None


def take_rows(x, pair_b, pair_q):
    """x [B, Q, ...] -> the M rows x[pair_b[m], pair_q[m]] as one contiguous tensor [M, ...].  The backward allocates the zero
    gradient in x's OWN memory order (a channels-last view stays one) and writes the M rows into it, so the full-size gradient is
    written once and reaches the producer of x without a layout copy.  x must be dense (no overlapping or broadcast strides)."""
    pb = torch.as_tensor(pair_b, dtype=torch.int64).reshape(-1).to(x.device)
    pq = torch.as_tensor(pair_q, dtype=torch.int64).reshape(-1).to(x.device)
    if pb.numel() != pq.numel():
        raise ValueError('take_rows: pair_b and pair_q must have one length')
    return TakeRowsFn.apply(x, pb, pq)
