"""torch.autograd.Function wrappers over the libtcct_hip.so C-ABI.

PyTorch here is plumbing only (device memory via the caching allocator, the current HIP stream, the autograd tape);
every arithmetic op of the hot path is a HIP kernel behind `tcct_amd._lib.lib`.  No CPU fallback exists: a CPU tensor
or a missing .so raises.  Activations are NHWC-contiguous (`[N,H,W,C]`, tokens `[B,N,C]` are the same memory).
"""
import os
import weakref

import torch

from ._lib import lib, dtype_code, TcctError, launch_on, F32, BF16  # noqa: F401

ACT = {None: 0, 'none': 0, 'lrelu': 1, 'hswish': 2, 'gelu': 3, 'sigmoid': 4, 'abs': 5}


class _ZeroPool:
    """One pre-zeroed buffer per training step for every accumulation output (BN/LN partial sums, parameter-gradient buffers that
    have no slot in the optimizer's flat gradient): ONE memset per step instead of ~270 hipMemsetAsync calls.  Active between
    `begin_step()` and `end_step()`; otherwise the entry points clear their outputs themselves."""

    def __init__(self):
        self.buf = None
        self.off = 0
        self.active = False
        self.frozen = False     # set once a hipGraph has captured a step that uses the pool (tcct_amd/graph.py)

    def begin(self, device, nbytes=8 << 20):
        if self.buf is None or self.buf.device != device or self.buf.numel() < nbytes:
            if self.frozen:     # a captured hipGraph holds pointers into the pool: replacing it would leave them dangling
                raise TcctError('the zero pool cannot be re-allocated after a training step was captured into a hipGraph '
                                f'(pool on {self.buf.device}, step on {device})')
            self.buf = torch.empty(nbytes, device=device, dtype=torch.uint8)
        self.buf.zero_()
        self.off = 0
        self.active = True
        lib.set_outputs_prezeroed(1)

    def end(self):
        if self.active:
            self.active = False
            lib.set_outputs_prezeroed(0)

    def get(self, shape, dtype, device):
        """zero-initialised tensor when the pool is active, uninitialised otherwise (the entry point clears it then)"""
        n = 1
        for d in shape:
            n *= d
        nbytes = n * dtype.itemsize
        if not self.active:
            return torch.empty(shape, device=device, dtype=dtype)
        start = (self.off + 255) // 256 * 256
        if self.buf.device != device or start + nbytes > self.buf.numel():
            return torch.zeros(shape, device=device, dtype=dtype)
        self.off = start + nbytes
        return self.buf[start:start + nbytes].view(dtype).view(shape)


ZERO = _ZeroPool()


# ---- one weight-pack launch per step (round 3) -----------------------------------------------------------------------------------------
# The bf16 [tap][co][ci] packs (+ the flipped / transposed input-gradient packs) of the ~40 dense 32 -> 32 convolutions used to be made by one
# small launch per convolution per step (39 x ~5 us on the critical stream).  Convolutions seen during a pooled step are remembered; from the
# next step on begin_step() re-packs ALL of them with one launch (the optimizer has just changed the weights) and the forward pass picks its
# pack out of the cache.  `PACK_ALL = False` (bench.py --set PACK_ALL=0) restores the per-call launches.
PACK_ALL = True
# ent: key -> [weakref(weight), pack buffer, (KH, KW, byte offset of the packed rows in the weight), data_ptr, step last looked up]; key = id(weight), or
# (id(weight), o) for the 32-output slab o of the 32 -> 64 stem convolution (_pack_lookup_wide).  Entries hold NO strong reference to the weight:
# a dead model's entries disappear at the next begin_step(), as do entries no convolution asked for during the previous step.
# frozen / keep: once a hipGraph has captured a step whose pack launch reads a descriptor table, that table and the pack buffers it names are kept
# alive for the life of the process (`keep`) -- a replay reads their addresses -- and a changed entry set builds a NEW table beside them.
_PACKS = {'ent': {}, 'desc': None, 'sig': None, 'fresh': False, 'step': 0, 'frozen': False, 'keep': []}


def packs_freeze():
    """called by tcct_amd.graph after a capture that contains the pack-all launch: pins the captured table and its pack buffers"""
    _PACKS['frozen'] = True
    if _PACKS['desc'] is not None:
        _PACKS['keep'].append((_PACKS['desc'], [e[1] for e in _PACKS['ent'].values()]))


def _pack_lookup(w, KH, KW):
    """(forward pack, input-gradient pack) of weight w made by this step's pack-all launch, or None"""
    if not (PACK_ALL and ZERO.active):
        return None
    ent = _PACKS['ent'].get(id(w))
    if ent is None or ent[0]() is not w or ent[3] != w.data_ptr() or ent[2] != (KH, KW, 0):
        wp2 = torch.empty(2 * KH * KW * 1024, device=w.device, dtype=torch.bfloat16)
        _PACKS['ent'][id(w)] = [weakref.ref(w), wp2, (KH, KW, 0), w.data_ptr(), _PACKS['step']]
        _PACKS['sig'] = None                    # the descriptor table is rebuilt at the next begin_step()
        return None
    ent[4] = _PACKS['step']
    if not _PACKS['fresh'] or _PACKS['sig'] is None or not ent[5:]:
        return None
    n = KH * KW * 1024
    return ent[1][:n], ent[1][n:]


def _pack_lookup_wide(w):
    """the 3x3 32 -> 64 weight (MPViT stem[1]) in the same registry: rows 32 o ..+31 of an OIHW [64, 32, 3, 3] weight are a contiguous [32, 32, 3, 3] weight of
    their own, so each output slab is one more record of the pack-all launch.  -> one buffer [slab o][forward pack, input-gradient pack][9 * 1024] made by this
    step's launch, or None"""
    if not (PACK_ALL and ZERO.active):
        return None
    n = 9 * 1024
    ents = [_PACKS['ent'].get((id(w), o)) for o in range(2)]
    if any(e is None or e[0]() is not w or e[3] != w.data_ptr() for e in ents) or ents[1][1].data_ptr() != ents[0][1].data_ptr() + 4 * n:
        buf = torch.empty(4 * n, device=w.device, dtype=torch.bfloat16)
        for o in range(2):
            _PACKS['ent'][(id(w), o)] = [weakref.ref(w), buf[2 * n * o:2 * n * (o + 1)], (3, 3, o * 32 * 32 * 9 * 4), w.data_ptr(), _PACKS['step']]
        _PACKS['sig'] = None
        return None
    for e in ents:
        e[4] = _PACKS['step']
    if not _PACKS['fresh'] or _PACKS['sig'] is None or not (ents[0][5:] and ents[1][5:]):
        return None
    return ents[0][1]._base


def _pack_evict():
    """drop entries whose weight is gone, whose storage was re-bound (the flat optimizer buffer, load_state_dict) or that no convolution of the
    previous step looked up (another model's step in between, a changed loss configuration)"""
    step = _PACKS['step']
    for k in [k for k, e in _PACKS['ent'].items() if e[0]() is None or e[0]().data_ptr() != e[3] or e[4] < step]:
        del _PACKS['ent'][k]
    _PACKS['step'] = step + 1


def _pack_all(device):
    ents = [e for e in _PACKS['ent'].values() if e[0]().device == device]
    _PACKS['fresh'] = False
    if not (PACK_ALL and ents):
        return
    sig = tuple((e[3] + e[2][2], e[1].data_ptr()) for e in ents)
    if sig != _PACKS['sig'] and torch.cuda.is_current_stream_capturing():
        return                      # the descriptor upload is a host-to-device copy: not inside a hipGraph capture (the convolutions pack per call then)
    if sig != _PACKS['sig']:
        rows = [[e[3] + e[2][2], e[1].data_ptr(), e[2][0], e[2][1]] for e in ents]
        _PACKS['desc'] = torch.tensor(rows, dtype=torch.int64).to(device)       # a NEW tensor: tables named by captured graphs stay in `keep`
        _PACKS['sig'] = sig
    for e in _PACKS['ent'].values():
        del e[5:]
    for e in ents:
        e.append(True)              # packed by this launch
    lib.conv32_pack_weights_multi(_PACKS['desc'], len(ents))
    _PACKS['fresh'] = True


BILINEAR_BWD_X2 = True      # exact x2 resizes: the separable lane-exchange backward (tcct_bilinear_bwd_x2; round 6); False: the tiled gather kernel (A/B timing)
_BILINEAR_X2_SET = [True]


def begin_step(device):
    """call once per training step before the forward (KiteSeg.train_step does): arms the zero pool"""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:          # torch.device('cuda') != torch.device('cuda', 0): never re-allocate the pool for that
        device = torch.device('cuda', torch.cuda.current_device())
    ZERO.begin(device)
    if BILINEAR_BWD_X2 != _BILINEAR_X2_SET[0]:          # kernel A/B (bench.py --set BILINEAR_BWD_X2=0): the library-wide switch follows the module constant
        lib.bilinear_bwd_x2(int(BILINEAR_BWD_X2))
        _BILINEAR_X2_SET[0] = BILINEAR_BWD_X2
    fpl_lazy_grad_reset()
    _pack_evict()
    _pack_all(device)
    _STEP['main'] = torch.cuda.current_stream(device)
    for v in _STEP['marks'].values():
        v[0] = v[1] = 0


# ---- gradient-readiness marks (data-parallel overlap, tcct_amd/dist.py) ------------------------------------------------------
# The optimizer of a data-parallel run all-reduces its flat gradient in buckets while the rest of the backward pass is still running
# (decoder/FTC -> deep encoder levels -> level 0).  A bucket is complete when the backward pass has crossed every
# tensor edge that leads out of its modules; the model marks those edges with grad_mark(x, key): identity in the forward, and its
# backward node reports "one more edge of `key` crossed".  Without a registered listener grad_mark is a no-op (single-GPU path).
_STEP = {'main': None, 'marks': {}, 'listener': None}


def set_grad_mark_listener(fn):
    """fn(key) is called (from autograd's device thread) when the backward pass has crossed ALL edges marked `key` in this step"""
    _STEP['listener'] = fn
    _STEP['marks'].clear()


def step_streams():
    """every stream this library may have launched kernels of the running step on: the step's main stream + the side streams"""
    out = [] if _STEP['main'] is None else [_STEP['main']]
    for v in _SIDE_STREAMS.values():
        out.append(v[0] if isinstance(v, tuple) else v)
    return out


class _FastFunction(torch.autograd.Function):
    """torch.autograd.Function whose `apply` goes straight to the C++ implementation (round 6).  `Function.apply` first checks for a `setup_context` override, asks whether
    functorch transforms are active and runs `unwrap_dead_wrappers` over the arguments -- 6-8 us per call, ~130 calls per forward pass; the forward pass of the bench step is
    HOST-bound (tools/host_profile.py: ~8 ms of enqueue for ~5.5 ms of kernels once the two encoders overlap), so this is step time, not bookkeeping.  None of these
    Functions defines `setup_context` or is used under functorch transforms (vmap / grad / jvp)."""

    @classmethod
    def apply(cls, *args):
        return super(torch.autograd.Function, cls).apply(*args)


class _GradMark(_FastFunction):
    @staticmethod
    def forward(ctx, x, key):
        ctx.key = key
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        cnt = _STEP['marks'].get(ctx.key)
        fn = _STEP['listener']
        if cnt is not None and fn is not None:
            cnt[1] += 1
            if cnt[1] == cnt[0]:
                fn(ctx.key)
        return dy, None


def grad_mark(x, key):
    if _STEP['listener'] is None or not ZERO.active or not (torch.is_grad_enabled() and x.requires_grad):
        return x
    _STEP['marks'].setdefault(key, [0, 0])[0] += 1
    y = _GradMark.apply(x, key)
    link = getattr(x, '_skip0', None)
    if link is not None:        # the alias is the same edge: a low-rank gradient recipe (SKIP0_LOWRANK) passes this node's backward untouched
        y._skip0 = link
    return y


def end_step():
    ZERO.end()
    if _WGRAD_USED:             # weight gradients were issued on the side stream: the optimizer (current stream) must see them
        cur = torch.cuda.current_stream()
        for st in _WGRAD_USED.values():
            cur.wait_stream(st)
        _WGRAD_USED.clear()
    _WGRAD_KEEP.clear()         # after the join: blocks freed from here on are reused by work ordered behind the weight gradients


# Weight-gradient kernels only feed the optimizer, so inside a pooled step they are issued on a side stream and joined in
# end_step(): the input-gradient chain (the critical path of backward) continues without waiting for them and the
# latency-bound weight gradients of the coarse levels overlap it.  TCCT_STREAMS=0 disables.
_WGRAD_USED = {}
_WGRAD_KEEP = []
DW_WGRAD_SIDE = True


def fresh_stream(device=None, avoid=()):
    """A torch.cuda.Stream whose HIP stream is none of: the current stream, the library's side streams, `avoid`.  torch hands out streams
    from a pool of 32 per device, round-robin: in a long process the 33rd `torch.cuda.Stream()` IS the first one again, and a capture
    stream that aliased the weight-gradient / encoder side stream would turn their fork-join into a wait of a stream on itself.  (A guard:
    it was written while chasing the late-capture segfault of DESIGN 5b, which it did NOT cure.)"""
    taken = {torch.cuda.current_stream(device).cuda_stream}
    for v in _SIDE_STREAMS.values():
        taken.add((v[0] if isinstance(v, tuple) else v).cuda_stream)
    for st in avoid:
        taken.add(st.cuda_stream)
    for _ in range(64):
        st = torch.cuda.Stream(device=device)
        if st.cuda_stream not in taken:
            return st
    raise TcctError('fresh_stream: no stream of the pool is free of aliases')


class _wgrad_stream:
    def __init__(self, enable, *tensors):
        self.enable, self.tensors = enable, tensors

    def __enter__(self):
        if not self.enable:
            return self
        cur = torch.cuda.current_stream()
        key = ('wgrad', cur.device.index)
        ent = _SIDE_STREAMS.get(key)
        if ent is None:         # the side stream and ONE reusable event for the cur -> side dependency (a wait captures the state of the
            ent = _SIDE_STREAMS[key] = (fresh_stream(cur.device), torch.cuda.Event())   # event at the time it is issued)
        self.side, ev = ent
        ev.record(cur)
        self.side.wait_event(ev)
        # the block only launches this library's kernels into pre-allocated gradient slots: name the stream for them instead of
        # re-binding torch's current stream (launch_on: ~1 us instead of ~25 us per weight gradient)
        self.ctx = launch_on(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if not self.enable:
            return False
        self.ctx.__exit__(*exc)
        # autograd may drop x / dy as soon as this node returns while the side stream still reads them.  They are kept alive until
        # end_step() has joined the side stream -- NOT tensor.record_stream(side): with every activation and gradient of the step
        # marked that way the caching allocator could not reuse a block until the side stream caught up, the host runs most of a
        # step ahead, and the reserved pool grew by ~3.5 GB per step (124 GB after 30 steps, then a multi-second free-and-retry stall)
        _WGRAD_KEEP.extend(self.tensors)
        _WGRAD_USED[id(self.side)] = self.side
        return False


def _slot_written(*params):
    return PARALLEL_BRANCHES and ZERO.active and all(p is None or getattr(p, '_grad_slot', None) is not None for p in params)


def _grad_out(param, shape=None):
    """destination of a parameter gradient: the parameter's slot in the optimizer's flat gradient buffer (pre-zeroed by
    zero_grad; written in place, so the optimizer needs no gather) or a pooled / fresh tensor"""
    slot = getattr(param, '_grad_slot', None)
    if slot is not None and ZERO.active:
        return slot.view(shape if shape is not None else slot.shape)
    return ZERO.get(tuple(shape if shape is not None else param.shape), torch.float32, param.device)


def _written_grad_out(param, n):
    """destination of a parameter gradient [n] that the kernel WRITES (the BatchNorm family's dgamma / dbeta): the parameter's slot, else an uninitialised
    tensor.  Not _grad_out: its fallback is a zeroed pool tensor, for kernels that accumulate -- here that would spend pool space on zeros nobody reads."""
    return _grad_out(param) if ZERO.active and getattr(param, '_grad_slot', None) is not None else torch.empty(n, device=param.device, dtype=torch.float32)


def _zeros(shape, dtype, device):
    """a zero-filled accumulation output: out of the step's pre-zeroed pool when one is active"""
    return ZERO.get(shape, dtype, device) if ZERO.active else torch.zeros(shape, device=device, dtype=dtype)


def _ret(t, param):
    """what a backward returns for a parameter gradient: None when the kernel already wrote it into the parameter's slot of the
    flat gradient buffer (autograd must not clone/accumulate it again; the optimizer reads the slot), else the tensor itself"""
    if t is None:
        return None
    slot = getattr(param, '_grad_slot', None)
    if slot is not None and t.data_ptr() == slot.data_ptr():
        return None
    return t


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise TcctError('tcct_amd ops need CUDA(HIP) tensors; there is no CPU fallback')
        if not t.is_contiguous():
            raise TcctError(f'non-contiguous tensor of shape {tuple(t.shape)} passed to a HIP op')


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _as(t, dtype):
    t = _c(t)
    return t if t.dtype == dtype else t.to(dtype)


# ------------------------------------------------------------------------------------------------- conv
# fp32 MFMA for the pointwise forward / input gradient / weight gradient.  The FORWARD stays on the sequential VALU kernel in the parity mode: on
# the formula-weight fixtures some BatchNorm channels at the 2x2 / 4x4 levels have a batch variance at fp32 rounding level, and the MFMA summation
# order (exact to 2-5e-7 against fp64, like the VALU kernel's) moved rstd enough to scale the whole CNN level-0 gradient by 0.93 -- outside the
# envelope the fixtures assert, which is built from oneDNN's sequential order (tests/test_model_gpu.py, profiles/r03_parity.md).  TCCT_F32_PW_FWD=1
# puts the forward on the matrix pipes as well (+~5 % fp32 throughput).
F32_PW = [os.environ.get('TCCT_F32_PW_FWD', '0') == '1', True, True]


# The 3x3 32 -> 64 convolution (MPViT stem[1], reference nets/tcct.py:682-689) as ONE launch per direction (tcct_conv32x64_fwd33 / tcct_conv64x32_dgrad33 /
# tcct_conv32x64_wgrad33: wave pairs per strip, x / dy read from HBM once, dx rounded once) with its packs out of the one-launch-per-step registry.  The forward is
# bit-identical to the slab path; TCCT_WIDE_CONV=0 restores the slab path (A/B timing).
WIDE_CONV = os.environ.get('TCCT_WIDE_CONV', '1') != '0'


def conv_route(in_dt, out_dt, Cin, Cin_w, Cout, KH, KW, stride, padh, padw):
    """The kernel family of a convolution, from dtypes and integers alone (no tensor, no device) -- every direction of _Conv2d and conv_bn_act resolve from it
    (conv_fwd_route / conv_dgrad_route / conv_wgrad_route), and a new family is one clause here plus one row of _CONV_ROUTES:
      pw         bf16 input, 1x1 / Linear, Cin % 32 == 0: the MFMA pointwise kernels (any output dtype)
      pwf        fp32 1x1 / Linear, Cin and Cout multiples of 32: the fp32 MFMA pointwise kernels (conv_f32_mfma.hip)
      c32        bf16 32 -> 32 stride-1 'same' 3x3 / 1xk / kx1: the MFMA implicit-GEMM kernel
      c32f       the same in fp32 (parity mode), k <= 13
      wide33     bf16 32 -> 64 3x3 (MPViT stem[1]) as one launch per direction; WIDE_CONV = False leaves it to `slabs`
      slabs      wider bf16 'same' convolutions (channel counts multiples of 32 up to 256, k <= 13) as 32x32 sub-GEMMs of the conv32 kernels: MPViT stem[1] and
                 the wide CNN encoder of stc_tb / gtc_tb (32-64-96-128-256, nets/tcct.py:861-864)
      slabs_f32  the same in fp32 (MPViT stem[1] 32->64 is a third of the parity mode's convolution time on the VALU kernel)
      generic    everything else: the VALU convolution"""
    if stride != 1 or Cin != Cin_w:
        return 'generic'
    if KH == 1 and KW == 1:
        if padh != 0 or padw != 0 or Cin % 32 != 0:
            return 'generic'
        if in_dt == torch.bfloat16:
            return 'pw'
        return 'pwf' if in_dt == torch.float32 and out_dt == torch.float32 and Cout % 32 == 0 else 'generic'
    if (in_dt != out_dt or in_dt not in (torch.bfloat16, torch.float32) or 2 * padh != KH - 1 or 2 * padw != KW - 1
            or not (KH == 1 or KW == 1 or (KH == 3 and KW == 3))):
        return 'generic'
    bf = in_dt == torch.bfloat16
    if Cin == 32 and Cout == 32:
        if bf:
            return 'c32'
        return 'c32f' if max(KH, KW) <= 13 else 'generic'
    if Cin % 32 != 0 or Cout % 32 != 0 or not (32 <= Cin <= 256 and 32 <= Cout <= 256) or max(KH, KW) > 13:
        return 'generic'
    if not bf:
        return 'slabs_f32'
    return 'wide33' if WIDE_CONV and Cin == 32 and Cout == 64 and KH == 3 and KW == 3 else 'slabs'


def conv_fwd_route(route):
    """the three directions take `route` = conv_route of the forward orientation (x's dtype in, the output's / dy's dtype out)"""
    return 'generic' if route == 'pwf' and not F32_PW[0] else route


def conv_dgrad_route(route, x_dt, dy_dt, Cin, Cin_w, Cout, KH, KW, stride, padh, padw):
    """the input gradient is the transposed convolution: dy -> dx with the roles of Cin and Cout swapped"""
    if stride != 1 or Cin != Cin_w:
        raise TcctError('conv2d dgrad: only stride-1 convs with unpadded channels need an input gradient')
    if route == 'wide33':
        return route
    t = conv_route(dy_dt, x_dt, Cout, Cout, Cin, KH, KW, stride, padh, padw)
    if (t == 'pw' and x_dt != torch.bfloat16) or (t == 'pwf' and not F32_PW[1]):
        return 'generic'
    return 'slabs' if t == 'wide33' else t          # 64 -> 32: the wide kernel only runs this way round as the gradient of 32 -> 64


def conv_wgrad_route(route, x_dt, dy_dt, Cin, Cin_w, Cout, KH, KW, stride, padh, padw):
    if route == 'pwf' and not (F32_PW[2] and Cout <= 160):
        route = 'generic'
    if route == 'pw':
        if dy_dt == torch.bfloat16 and Cout % 32 == 0:
            # wider outputs (the qkv Linear of the factorised attention, Cout = 3 dim): slabs of <= 160 columns on the same kernel
            return 'pw' if Cout <= 160 else 'pw_strided'
        route = 'generic'
    if (route == 'generic' and KH == 1 and KW == 1 and stride == 1 and Cout <= 8 and Cin == Cin_w and Cin <= 256
            and (x_dt == torch.bfloat16 or dy_dt == torch.float32)):
        return 'smalln'
    return route


def _wide_packs(w):
    """[slab o][forward pack, input-gradient pack][9 * 1024] bf16 of an OIHW [64, 32, 3, 3] weight: this step's pack-all launch, else one launch per slab"""
    buf = _pack_lookup_wide(w)
    if buf is None:
        buf = torch.empty(4 * 9 * 1024, device=w.device, dtype=torch.bfloat16)
        for o in range(2):
            lib.conv32_pack_weights_both(w[32 * o:], buf[2 * 9 * 1024 * o:], 3, 3)
    return buf


def _conv_slabs_fwd(x, w, bias, y, N, H, W, Cin, Cout, KH, KW, padh, padw, transposed, stats=None, stat_pre=0):
    """y[..., Cout] = conv(x[..., Cin]) via 32x32 sub-GEMMs of the conv32 kernels (bf16) / the fp32 MFMA kernels (no fused statistics there); transposed=True
    computes the input gradient (x=dy, w OIHW [Cin_orig=Cout here][...]) i.e. roles of the weight's O/I dims swap"""
    pack, fwd = (lib.conv32_pack_weights_sub, lib.conv32_fwd_strided) if x.dtype == torch.bfloat16 else (lib.conv32f_pack_weights_sub, lib.conv32f_fwd_strided)
    for oh in range(Cout // 32):
        for ih in range(Cin // 32):
            wp = torch.empty(KH * KW * 1024, device=x.device, dtype=x.dtype)
            if not transposed:
                pack(w, wp, KH, KW, 0, Cin, 32 * oh, 32 * ih)
            else:       # w is OIHW [Cin(this call's input = orig Cout)][Cout(this call's output = orig Cin)]
                pack(w, wp, KH, KW, 1, Cout, 32 * ih, 32 * oh)
            b = bias[32 * oh:32 * oh + 32] if (bias is not None and ih == 0) else None
            if stats is not None and ih == Cin // 32 - 1:       # the last input slab: the accumulated output is what the BatchNorm statistics count
                lib.conv32_fwd_strided_bnstats(x, wp, b, y, N, H, W, KH, KW, padh, padw, Cin, 32 * ih, Cout, 32 * oh, 1 if ih > 0 else 0, stats, stat_pre)
            else:
                fwd(x, wp, b, y, N, H, W, KH, KW, padh, padw, Cin, 32 * ih, Cout, 32 * oh, 1 if ih > 0 else 0)


def _pw_bwd_ok(x, dy, Cin, Cin_w, Cout, KH, KW, stride, padh, padw):
    """shapes of the fused pointwise backward kernel (tcct_pw_bwd): bf16 1x1, channel counts in {32, 64, 96, 128}"""
    return (x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16 and KH == 1 and KW == 1 and stride == 1 and padh == 0 and padw == 0
            and Cin == Cin_w and Cin % 32 == 0 and Cout % 32 == 0 and 32 <= Cin <= 128 and 32 <= Cout <= 128
            and x.numel() * 2 < 2 ** 31 and dy.numel() * 2 < 2 ** 31)


def _packs32(w, KH, KW, need_t):
    """(forward pack, input-gradient pack or None) of a 32 -> 32 weight: this step's pack-all launch (begin_step), or packed here -- with need_t both packs
    out of one launch"""
    cached = _pack_lookup(w, KH, KW)
    if cached is not None:
        return cached
    n = KH * KW * 1024
    if need_t:
        wp2 = torch.empty(2 * n, device=w.device, dtype=torch.bfloat16)
        lib.conv32_pack_weights_both(w, wp2, KH, KW)
        return wp2[:n], wp2[n:]
    wp = torch.empty(n, device=w.device, dtype=torch.bfloat16)
    lib.conv32_pack_weights(w, wp, KH, KW, 0)
    return wp, None


def _pack_t(wp_t, w, KH, KW):
    """the input-gradient pack the forward left behind, or packed here"""
    if wp_t is None:
        wp_t = torch.empty(KH * KW * 1024, device=w.device, dtype=torch.bfloat16)
        lib.conv32_pack_weights(w, wp_t, KH, KW, 1)
    return wp_t


# ---- the launchers of every route: forward(ctx, x, w, bias, y, stats_box, g), input gradient(ctx, dy, w, dskip, dx, g) -> the dskip still to be added (None
# when the kernel's epilogue took it), weight gradient(x, dy, dw, db, g); g = (N, H, W, Cin, Cin_w, Cout, KH, KW, stride, padh, padw) of the FORWARD
def _stat_sums(stats_box, C, device):
    """pre-zeroed [sum | sum of squares] of the consumer's train-mode BatchNorm (stats_box = [pre_act_code, None]), or None"""
    if stats_box is None:
        return None, 0
    stats_box[1] = _zeros((2 * C,), torch.float64, device)
    return stats_box[1], stats_box[0]


def _stats_box(stats_pre):
    """[pre-activation code, None] for a node whose kernel may accumulate the statistics of the train-mode BatchNorm behind it (slot 1 receives them), or None"""
    return [ACT[stats_pre], None] if stats_pre is not None else None


def _tag_bn_sums(y, box):
    """the node filled its box: y carries (sums, pre-activation code) as `_bn_sums`, which _bn_batch_sums takes instead of running tcct_bn_stats"""
    if box is not None and box[1] is not None:
        y._bn_sums = (box[1], box[0])
    return y


def _clear_unless_prezeroed(dw, db):
    """in front of kernels that accumulate into dw / db: inside a pooled step the gradient slots and the pool are already zero"""
    if not ZERO.active:
        dw.zero_()
        if db is not None:
            db.zero_()


def _fwd_pw(ctx, x, w, bias, y, stats_box, g):
    N, H, W, Cin, _, Cout = g[:6]
    if stats_box is not None and y.dtype == torch.bfloat16 and Cout % 32 == 0 and Cout <= 160:
        sums, pre = _stat_sums(stats_box, Cout, x.device)
        lib.pw_fwd_bnstats(x, w, bias, y, N * H * W, Cin, Cout, sums, pre)
    else:
        lib.pw_fwd(x, w, bias, y, N * H * W, Cin, Cout, 0, dtype_code(y.dtype))


def _dgrad_pw(ctx, dy, w, dskip, dx, g):
    N, H, W, Cin, _, Cout = g[:6]
    if dskip is not None and Cin % 32 == 0:
        lib.pw_dgrad_residual(dy, w, dskip, dx, None, N * H * W, Cout, Cin)
        return None
    lib.pw_fwd(dy, w, None, dx, N * H * W, Cout, Cin, 1, dtype_code(dx.dtype))
    return dskip


def _wgrad_pw(x, dy, dw, db, g):
    N, H, W, Cin, _, Cout = g[:6]
    (lib.pw_wgrad if x.dtype == torch.bfloat16 else lib.pwf_wgrad)(x, dy, dw, db, N * H * W, Cin, Cout)


def _wgrad_pw_strided(x, dy, dw, db, g):
    N, H, W, Cin, _, Cout = g[:6]
    dy2, dw2 = dy.view(-1, Cout), dw.view(Cout, Cin)
    for c0 in range(0, Cout, 160):
        n = min(160, Cout - c0)
        lib.pw_wgrad_strided(x, dy2[0, c0:], Cout, dw2[c0:], db[c0:] if db is not None else None, N * H * W, Cin, n)


def _wgrad_smalln(x, dy, dw, db, g):
    N, H, W, Cin, _, Cout = g[:6]
    lib.pw_wgrad_smalln(x, dy, dw, db, N * H * W, Cin, Cout, dtype_code(x.dtype), dtype_code(dy.dtype))


def _fwd_pwf(ctx, x, w, bias, y, stats_box, g):
    N, H, W, Cin, _, Cout = g[:6]
    lib.pwf_fwd(x, w, bias, y, N * H * W, Cin, Cout, 0)


def _dgrad_pwf(ctx, dy, w, dskip, dx, g):
    N, H, W, Cin, _, Cout = g[:6]
    lib.pwf_fwd(dy, w, None, dx, N * H * W, Cout, Cin, 1)
    return dskip


def _fwd_wide33(ctx, x, w, bias, y, stats_box, g):
    N, H, W = g[:3]
    sums, pre = _stat_sums(stats_box, 64, x.device)
    ctx.wp_wide = _wide_packs(w)
    lib.conv32x64_fwd33(x, ctx.wp_wide, 2 * 9 * 1024, bias, y, N, H, W, sums, pre, 0)


def _dgrad_wide33(ctx, dy, w, dskip, dx, g):
    N, H, W = g[:3]
    lib.conv64x32_dgrad33(dy, ctx.wp_wide[9 * 1024:], 2 * 9 * 1024, dx, N, H, W, 0)      # the packs the forward of this route left behind
    return dskip


def _wgrad_wide33(x, dy, dw, db, g):
    N, H, W = g[:3]
    _clear_unless_prezeroed(dw, db)
    lib.conv32x64_wgrad33(x, dy, dw, db, N, H, W, 0)


def _fwd_slabs(ctx, x, w, bias, y, stats_box, g):
    N, H, W, Cin, _, Cout, KH, KW, _, padh, padw = g
    sums, pre = _stat_sums(stats_box if x.dtype == torch.bfloat16 else None, Cout, x.device)
    _conv_slabs_fwd(x, w, bias, y, N, H, W, Cin, Cout, KH, KW, padh, padw, False, sums, pre)


def _dgrad_slabs(ctx, dy, w, dskip, dx, g):
    N, H, W, Cin, _, Cout, KH, KW, _, padh, padw = g
    _conv_slabs_fwd(dy, w, None, dx, N, H, W, Cout, Cin, KH, KW, KH - 1 - padh, KW - 1 - padw, True)
    return dskip


def _wgrad_slabs(x, dy, dw, db, g):
    N, H, W, Cin, _, Cout, KH, KW, _, padh, padw = g
    wgrad_strided = lib.conv32_wgrad_strided if x.dtype == torch.bfloat16 else lib.conv32f_wgrad_strided
    _clear_unless_prezeroed(dw, db)
    for oh in range(Cout // 32):
        for ih in range(Cin // 32):
            wgrad_strided(x, dy, dw, db if ih == 0 else None, N, H, W, KH, KW, padh, padw, Cin, 32 * ih, Cout, 32 * oh, Cin, 32 * oh, 32 * ih)


def _fwd_c32(ctx, x, w, bias, y, stats_box, g):
    N, H, W, _, _, _, KH, KW, _, padh, padw = g
    wp, ctx.wp_t = _packs32(w, KH, KW, ctx.needs_input_grad[0])
    if stats_box is not None:
        sums, pre = _stat_sums(stats_box, 32, x.device)
        lib.conv32_fwd_bnstats(x, wp, bias, y, N, H, W, KH, KW, padh, padw, sums, pre)
    else:
        lib.conv32_fwd(x, wp, bias, y, N, H, W, KH, KW, padh, padw)


def _dgrad_c32(ctx, dy, w, dskip, dx, g):
    N, H, W, _, _, _, KH, KW, _, padh, padw = g
    wp = _pack_t(ctx.wp_t, w, KH, KW)
    if dskip is not None:
        lib.conv32_fwd_add(dy, wp, None, dskip, dx, N, H, W, KH, KW, KH - 1 - padh, KW - 1 - padw)
    else:
        lib.conv32_fwd(dy, wp, None, dx, N, H, W, KH, KW, KH - 1 - padh, KW - 1 - padw)
    return None


def _wgrad_c32(x, dy, dw, db, g):
    N, H, W, _, _, _, KH, KW, _, padh, padw = g
    (lib.conv32_wgrad if x.dtype == torch.bfloat16 else lib.conv32f_wgrad)(x, dy, dw, db, N, H, W, KH, KW, padh, padw)


def _fwd_c32f(ctx, x, w, bias, y, stats_box, g):
    N, H, W, _, _, _, KH, KW, _, padh, padw = g
    wp = torch.empty(KH * KW * 1024, device=x.device, dtype=torch.float32)
    lib.conv32f_pack_weights(w, wp, KH, KW, 0)
    lib.conv32f_fwd(x, wp, bias, None, y, N, H, W, KH, KW, padh, padw)


def _dgrad_c32f(ctx, dy, w, dskip, dx, g):
    N, H, W, _, _, _, KH, KW, _, padh, padw = g
    wp = torch.empty(KH * KW * 1024, device=dy.device, dtype=torch.float32)
    lib.conv32f_pack_weights(w, wp, KH, KW, 1)
    lib.conv32f_fwd(dy, wp, None, dskip, dx, N, H, W, KH, KW, KH - 1 - padh, KW - 1 - padw)
    return None


def _fwd_generic(ctx, x, w, bias, y, stats_box, g):
    lib.conv2d_fwd(x, w, bias, y, *g, dtype_code(x.dtype), dtype_code(y.dtype))


def _dgrad_generic(ctx, dy, w, dskip, dx, g):
    N, _, _, Cin, _, Cout, KH, KW, _, padh, padw = g
    # the entry takes the extent of its INPUT, dy [N, Ho, Wo, Cout]: the forward's H x W only for 'same' convolutions (an even K, a padded 1x1: Ho != H)
    lib.conv2d_dgrad(dy, w, dx, N, dy.shape[1], dy.shape[2], Cin, Cout, KH, KW, padh, padw, dtype_code(dy.dtype), dtype_code(dx.dtype))
    return dskip


def _wgrad_generic(x, dy, dw, db, g):
    lib.conv2d_wgrad(x, dy, dw, db, *g, dtype_code(x.dtype), dtype_code(dy.dtype))


# route -> (forward, input gradient, weight gradient); `pw_strided` and `smalln` only exist as weight gradients (conv_wgrad_route)
_CONV_ROUTES = {
    'pw': (_fwd_pw, _dgrad_pw, _wgrad_pw),
    'pwf': (_fwd_pwf, _dgrad_pwf, _wgrad_pw),
    'wide33': (_fwd_wide33, _dgrad_wide33, _wgrad_wide33),
    'slabs': (_fwd_slabs, _dgrad_slabs, _wgrad_slabs),
    'slabs_f32': (_fwd_slabs, _dgrad_slabs, _wgrad_slabs),            # the same loops: the slab helpers pick the kernels by dtype
    'c32': (_fwd_c32, _dgrad_c32, _wgrad_c32),
    'c32f': (_fwd_c32f, _dgrad_c32f, _wgrad_c32),
    'generic': (_fwd_generic, _dgrad_generic, _wgrad_generic),
    'pw_strided': (None, None, _wgrad_pw_strided),
    'smalln': (None, None, _wgrad_smalln),
}


def _param_of(w):
    """the parameter behind a weight: w may be a view of the nn.Linear weight (conv2d wrapper) -> gradient destinations look through ._base"""
    return w if hasattr(w, '_grad_slot') or w._base is None else w._base


class _Conv2d(_FastFunction):
    @staticmethod
    def forward(ctx, x, w, bias, stride, padh, padw, out_dtype, stats_box, fork=False):
        """fork: also return an alias of x for the OTHER consumers of x -- their gradient then arrives in backward() and is added
        inside the input-gradient kernel's epilogue (tcct_conv32_fwd_add) instead of by an autograd accumulation pass"""
        ctx.set_materialize_grads(False)      # an unused output must arrive as None in backward(), not as a zero-filled tensor
        _chk(x, w, bias)
        N, H, W, Cin = x.shape
        Cout, Cin_w, KH, KW = w.shape
        Ho = (H + 2 * padh - KH) // stride + 1
        Wo = (W + 2 * padw - KW) // stride + 1
        odt = out_dtype or x.dtype
        y = torch.empty((N, Ho, Wo, Cout), device=x.device, dtype=odt)
        shape = (Cin, Cin_w, Cout, KH, KW, stride, padh, padw)
        ctx.route = conv_route(x.dtype, odt, *shape)            # classified once: backward() resolves its two directions from it
        ctx.geom = (N, H, W) + shape
        _CONV_ROUTES[conv_fwd_route(ctx.route)][0](ctx, x, w, bias, y, stats_box, ctx.geom)
        ctx.save_for_backward(x, w)
        ctx.params = (_param_of(w), bias)
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, w = ctx.saved_tensors
        wsrc, bsrc = ctx.params
        if dy is None:          # only the alias was used downstream
            return dskip, None, None, None, None, None, None, None, None
        dy = _c(dy)
        if dskip is not None:
            dskip = _as(dskip, x.dtype)
        g = ctx.geom
        N, H, W = g[:3]
        shape = Cin, Cin_w, Cout, KH, KW, stride, padh, padw = g[3:]
        dx = dw = db = None
        if (ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and _pw_bwd_ok(x, dy, *shape) and (dskip is None or dskip.shape == x.shape)):
            # 1x1 convolution: input gradient, weight gradient and bias gradient in ONE pass over dy (tcct_pw_bwd); a second
            # consumer's gradient of x (fork) rides on the dx epilogue
            dx = torch.empty_like(x)
            dw = _grad_out(wsrc, tuple(w.shape))
            db = _grad_out(bsrc) if bsrc is not None else None
            lib.pw_bwd(x, dy, w, dskip, dx, dw, db, N * H * W, Cin, Cout)
            return dx, _ret(dw, wsrc), _ret(db, bsrc), None, None, None, None, None, None
        if ctx.needs_input_grad[0]:
            route = conv_dgrad_route(ctx.route, x.dtype, dy.dtype, *shape)
            dx = torch.empty_like(x)
            dskip = _CONV_ROUTES[route][1](ctx, dy, w, dskip, dx, g)
            if dskip is not None:       # kernels without the fused epilogue: one explicit pass
                tot = torch.empty_like(dx)
                lib.add(dx, dskip, tot, tot.numel(), dtype_code(tot.dtype))
                dx = tot
        elif dskip is not None:
            dx = dskip
        if ctx.needs_input_grad[1] or (bsrc is not None and ctx.needs_input_grad[2]):
            with _wgrad_stream(_slot_written(wsrc, bsrc), x, dy):
                dw = _grad_out(wsrc, tuple(w.shape))
                db = _grad_out(bsrc) if bsrc is not None else None
                _CONV_ROUTES[conv_wgrad_route(ctx.route, x.dtype, dy.dtype, *shape)][2](x, dy, dw, db, g)
        return dx, _ret(dw, wsrc), _ret(db, bsrc), None, None, None, None, None, None


def conv2d_fork(x, w, bias=None, stride=1, pad=0, stats_pre=None):
    """(conv2d(x), x'): x' aliases x and is to be read by the other consumers of x (see _Conv2d.forward `fork`)"""
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    if not (torch.is_grad_enabled() and x.requires_grad and x.dim() == 4):
        return conv2d(x, w, bias, stride, pad, stats_pre=stats_pre), x
    box = _stats_box(stats_pre)
    y, alias = _Conv2d.apply(x, w, bias, stride, ph, pw, None, box, True)
    return _tag_bn_sums(y, box), alias


def conv2d(x, w, bias=None, stride=1, pad=0, out_dtype=None, stats_pre=None):
    """x [N,H,W,Cin] (or tokens [B,N,C]); w OIHW fp32 (or [Cout,Cin] for nn.Linear).
    stats_pre: None, or the pre-activation name ('none', 'lrelu', ...) of a train-mode BatchNorm that consumes the output: kernels
    that can, accumulate the BN statistics in their epilogue and tag the result (`_bn_sums`) so `batchnorm` skips its own pass."""
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    tok = x.dim() == 3
    if tok:
        x = x.unsqueeze(2)
    if w.dim() == 2:
        w = w.view(w.shape[0], w.shape[1], 1, 1)
    box = _stats_box(stats_pre)
    y = _Conv2d.apply(x, w, bias, stride, ph, pw, out_dtype, box, False)
    if tok:
        y = y.squeeze(2)
    return _tag_bn_sums(y, box)


# ---- conv3x3 -> conv3x3 with nothing between them as ONE launch each way (round 5, csrc/conv_chain.hip) ---------------------------------------
# CrossCNNBlock.block12 (reference nets/tcct.py:808-810).  Forward: the intermediate is written once (the backward pass needs it) and not read back;
# backward: the input-gradient chain dy -> d mid -> dx the same way (d mid is the dy operand of the first convolution's weight gradient).  Results
# bit-identical to the two-launch path (TCCT_CONV_CHAIN=0), so no rounding point moves.
CONV_CHAIN = os.environ.get('TCCT_CONV_CHAIN', '1') != '0'
# Levels 0-1 only: on the small maps two launches of the tiled kernel are faster than one row-stream chain (8 x 200 x 276: 0.037 vs 0.040 ms,
# 8 x 100 x 138: 0.017 vs 0.029; `tools/chain_bench.py`) -- a wave walking down a strip is a long serial chain, and the small maps have few strips
CHAIN_MIN_PIXELS = 1 << 20


def conv3x3_chain_ok(x, w1, b1, w2, b2, stride1, pad1, stride2, pad2):
    return (CONV_CHAIN and x.dim() == 4 and x.dtype == torch.bfloat16 and x.is_cuda and x.shape[-1] == 32 and torch.is_grad_enabled()
            and tuple(w1.shape) == (32, 32, 3, 3) and tuple(w2.shape) == (32, 32, 3, 3) and stride1 == 1 and stride2 == 1
            and tuple(pad1) == (1, 1) and tuple(pad2) == (1, 1) and x.shape[1] * x.shape[2] * 64 < 2 ** 31
            and x.shape[0] * x.shape[1] * x.shape[2] >= CHAIN_MIN_PIXELS)


class _ConvChain33(_FastFunction):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, stats_box, fork):
        ctx.set_materialize_grads(False)
        _chk(x, w1, b1, w2, b2)
        N, H, W, _ = x.shape
        mid, y = torch.empty_like(x), torch.empty_like(x)
        need_t = ctx.needs_input_grad[0]
        wp1, ctx.wp_t1 = _packs32(w1, 3, 3, need_t)
        wp2, ctx.wp_t2 = _packs32(w2, 3, 3, True)             # d mid is always needed: it is the dy operand of the first convolution's weight gradient
        sums = None
        if stats_box is not None:
            sums = _zeros((64,), torch.float64, x.device)
            stats_box[1] = sums
        lib.conv32_chain33(x, wp1, b1, mid, wp2, b2, y, None, N, H, W, sums)
        ctx.save_for_backward(x, mid, w1, w2)
        ctx.params = (w1, b1, w2, b2)
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, mid, w1, w2 = ctx.saved_tensors
        p1, pb1, p2, pb2 = ctx.params
        if dy is None:          # only the alias was used downstream
            return dskip, None, None, None, None, None, None
        dy = _c(dy)
        N, H, W, _ = x.shape
        # what is asked for (a frozen block12 must neither cost two full-resolution weight-gradient passes nor have its slots in the flat gradient
        # buffer written -- AdamW would step a frozen parameter): as _Conv2d.backward, by ctx.needs_input_grad
        nx, nw1, nb1, nw2, nb2 = ctx.needs_input_grad[:5]
        g1, g2 = nw1 or (pb1 is not None and nb1), nw2 or (pb2 is not None and nb2)
        need_mid = nx or g1             # d mid feeds the input-gradient chain and the first convolution's weight gradient
        dx = dmid = None
        if need_mid:
            wt2 = _pack_t(ctx.wp_t2, w2, 3, 3)
            dmid = torch.empty_like(x) if g1 else None          # nobody reads d mid when the first convolution is frozen: the chain does not store it
            if nx:
                wt1 = _pack_t(ctx.wp_t1, w1, 3, 3)
                dx = torch.empty_like(x)
                lib.conv32_chain33(dy, wt2, None, dmid, wt1, None, dx, _as(dskip, x.dtype) if dskip is not None else None, N, H, W, None)
            else:
                lib.conv32_fwd(dy, wt2, None, dmid, N, H, W, 3, 3, 1, 1)
                dx = dskip
        else:
            dx = dskip
        dw1 = db1 = dw2 = db2 = None
        if g1 or g2:
            with _wgrad_stream(_slot_written(p1 if g1 else None, pb1 if g1 else None, p2 if g2 else None, pb2 if g2 else None),
                               *[t for t in (x, mid, dy, dmid) if t is not None]):
                if g2:
                    dw2, db2 = _grad_out(p2, tuple(w2.shape)), (_grad_out(pb2) if pb2 is not None else None)
                    lib.conv32_wgrad(mid, dy, dw2, db2, N, H, W, 3, 3, 1, 1)
                if g1:
                    dw1, db1 = _grad_out(p1, tuple(w1.shape)), (_grad_out(pb1) if pb1 is not None else None)
                    lib.conv32_wgrad(x, dmid, dw1, db1, N, H, W, 3, 3, 1, 1)
        return dx, _ret(dw1, p1), _ret(db1, pb1), _ret(dw2, p2), _ret(db2, pb2), None, None


def conv3x3_chain_infer_ok(x, w1, w2, stride1, pad1, stride2, pad2):
    return (CONV_CHAIN and INFER_FUSE and not torch.is_grad_enabled() and x.dim() == 4 and x.dtype == torch.bfloat16 and x.is_cuda and x.shape[-1] == 32
            and tuple(w1.shape) == (32, 32, 3, 3) and tuple(w2.shape) == (32, 32, 3, 3) and stride1 == 1 and stride2 == 1
            and tuple(pad1) == (1, 1) and tuple(pad2) == (1, 1) and x.shape[1] * x.shape[2] * 64 < 2 ** 31
            and x.shape[0] * x.shape[1] * x.shape[2] >= CHAIN_MIN_PIXELS)


def conv3x3_chain_infer(x, w1, b1, w2, b2):
    """inference (no_grad): conv3x3(conv3x3(x)) with the intermediate never written (check conv3x3_chain_infer_ok first)"""
    _chk(x, w1, b1, w2, b2)
    N, H, W, _ = x.shape
    y = torch.empty_like(x)
    wp = torch.empty(2 * 9 * 1024, device=x.device, dtype=torch.bfloat16)
    lib.conv32_pack_weights(w1, wp[:9 * 1024], 3, 3, 0)
    lib.conv32_pack_weights(w2, wp[9 * 1024:], 3, 3, 0)
    lib.conv32_chain33(x, wp[:9 * 1024], b1, None, wp[9 * 1024:], b2, y, None, N, H, W, None)
    return y


def conv3x3_chain(x, w1, b1, w2, b2, stats_pre=None, fork=False):
    """conv3x3(conv3x3(x; w1, b1); w2, b2), both 32 -> 32 'same' (check conv3x3_chain_ok first).  stats_pre: None or 'lrelu' (the train-mode BatchNorm that
    consumes the output: its statistics come out of the same launch, `_bn_sums`).  fork: also return an alias of x for the OTHER consumers of x, whose
    gradient is then added inside the input-gradient chain's epilogue."""
    if stats_pre not in (None, 'lrelu'):
        raise TcctError('conv3x3_chain: fused statistics only behind LeakyReLU')
    box = _stats_box(stats_pre)
    if fork and x.requires_grad:
        y, alias = _ConvChain33.apply(x, w1, b1, w2, b2, box, True)
    else:
        y, alias = _ConvChain33.apply(x, w1, b1, w2, b2, box, False), x
    _tag_bn_sums(y, box)
    return (y, alias) if fork else y


# The two encoders (CNN / ViT) only share the input and are issued on separate HIP streams:
# the launch-latency-bound kernels of the coarse levels then overlap other work instead of running one after another on an
# otherwise idle chip (-2.5 ms/step; forking block12/block34 and InvRes/token-mixer
# as well gained nothing more).  Autograd replays every node on the stream of its forward, so
# the backward pass overlaps the same way.  TCCT_STREAMS=0 issues everything on one stream.
PARALLEL_BRANCHES = os.environ.get('TCCT_STREAMS', '1') != '0'
# round 6: inside an MHCA stage whose maps have at most this many pixels (B*H*W) the transformer half runs on its own stream beside the InvRes half
# (MHCA_stage.forward); 0 disables.  tools/attrib_trace.sh: ViT L3-L4 are 2.4 ms of back-to-back 10-40 us launches in one stream -- but the fork pays at EVERY
# stage (same-box A/B, ms per step: stages 2-3 only 21.31 -> 21.05; + stage 1 20.94 -> 20.78; all four 20.97 -> 20.67): the depthwise kernels of one half are
# VALU-bound, the GEMMs of the other bandwidth-bound, and they fill each other's gaps.  Default: every stage.
STAGE_FORK_MAX_PIXELS = 1 << 30


FUSION_FORK = True       # FTC.forward: tran_vit / tran_cnn fusion of levels 1-2 on its own stream beside levels 3-4 + head (training, bench-like shapes)


def fusion_fork_ok(c5):
    """c5: the coarsest CNN level [B,h,w,32].  Small crops are launch-bound on the HOST: another fork / join there costs more than it gives"""
    return (FUSION_FORK and STAGE_FORK_MAX_PIXELS > 0 and PARALLEL_BRANCHES and torch.is_grad_enabled() and c5.is_cuda
            and c5.shape[0] * c5.shape[1] * c5.shape[2] >= FUSION_FORK_MIN_PIXELS)


FUSION_FORK_MIN_PIXELS = 4096       # coarsest level of 8 x 256 x 256 crops: 2048


def graphs_exclude_stage_fork(what):
    """hipGraph capture and the nested stage fork exclude each other in one process: a graph captured AFTER the fork's stream has been used crashes inside
    hipGraphLaunch at its first replay on ROCm 7.2 (tests/test_model_gpu.py::test_graphed_train_step_matches_eager; the same late-capture segfault as
    profiles/HISTORY.md 5b, now with a trigger that reproduces).  tcct_amd.graph calls this before a capture: the fork is switched off for the rest of the
    process, and a process that has already used it is refused loudly instead of crashing later."""
    global STAGE_FORK_MAX_PIXELS
    if any(k[0] == 'vit_enc' for k in _SIDE_STREAMS):
        raise TcctError(f'{what}: this process has already run training steps with the nested stage fork (tcct_amd.ops.STAGE_FORK_MAX_PIXELS > 0); a hipGraph '
                        'captured now crashes in hipGraphLaunch (DESIGN 6).  Set tcct_amd.ops.STAGE_FORK_MAX_PIXELS = 0 before the first step (KiteSeg does with '
                        '--graph=true / TCCT_GRAPH=1) or capture in a fresh process.')
    STAGE_FORK_MAX_PIXELS = 0
_SIDE_STREAMS = {}


def _tensors(o):
    if torch.is_tensor(o):
        yield o
    elif isinstance(o, (list, tuple)):
        for e in o:
            yield from _tensors(e)


def run_parallel(tag, fa, fb):
    """(fa(), fb()) with fb issued on the side stream `tag` and joined before returning"""
    if not (PARALLEL_BRANCHES and torch.cuda.is_available()):
        return fa(), fb()
    cur, side = torch.cuda.current_stream(), side_stream(tag)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        rb = fb()
    ra = fa()
    cur.wait_stream(side)
    # inside a pooled training step: keep what was allocated on the side stream and is consumed on the current one alive until end_step() instead of
    # record_stream()ing it -- every later piece of side-stream work starts behind a `side.wait_stream(cur)`, i.e. behind the readers, so a block freed after
    # the step's end cannot be overwritten early; record_stream() parks a freed block until the host-side event query sees the GPU catch up, and with the
    # host a third of a step ahead the reserved pool grew by 0.4 GB per step (tests/test_fullsize_gpu.py::test_allocator_pool_stays_bounded_over_steps_fullsize)
    keep_until_end_of_step(*_tensors(rb), cur)
    return ra, rb


def side_stream(tag):
    """the library's side stream `tag` of the current device (created on first use)"""
    cur = torch.cuda.current_stream()
    side = _SIDE_STREAMS.get((tag, cur.device.index))
    if side is None:
        side = _SIDE_STREAMS[(tag, cur.device.index)] = fresh_stream(cur.device)
    return side


def keep_until_end_of_step(*tensors_and_stream):
    """tensors allocated on a side stream and consumed on `stream` (the last argument): kept alive until end_step() inside a pooled step, record_stream()ed otherwise
    (see run_parallel)"""
    *ts, stream = tensors_and_stream
    if ZERO.active:
        _WGRAD_KEEP.extend(ts)
    else:
        for t in ts:
            t.record_stream(stream)


def run_interleaved(tag, ga, gb, outs_b):
    """Exhaust the generators ga (current stream) and gb (side stream `tag`) ALTERNATELY, gb first, and join.  The two encoders are
    issued level by level in turn rather than one after the other: the runtime lets the host run only a bounded number of launches
    ahead of the GPU, so with `ViT then CNN` the second stream received its first kernel when the first was nearly done, and -- autograd
    replays nodes in reverse creation order -- the backward pass ran the CNN encoder completely before the first ViT kernel.  Alternating
    creation order keeps both streams fed in both passes.  outs_b: the list gb fills (its tensors are handed to the current stream)."""
    if not (PARALLEL_BRANCHES and torch.cuda.is_available()):
        for _ in gb:
            pass
        for _ in ga:
            pass
        return
    cur, side = torch.cuda.current_stream(), side_stream(tag)
    side.wait_stream(cur)
    done_a = done_b = False
    end = object()
    while not (done_a and done_b):
        if not done_b:
            with torch.cuda.stream(side):
                done_b = next(gb, end) is end
        if not done_a:
            done_a = next(ga, end) is end
    cur.wait_stream(side)
    for t in _tensors(outs_b):
        t.record_stream(cur)        # allocated on the side stream, consumed on the current one


INFER_FUSE = True       # eval-mode forward under no_grad folds BatchNorm / activations into the convolution epilogues (False: op by op)


def conv_bn_act(x, w, bias=None, stride=1, pad=0, bn=None, pre_act=None, post_act=None):
    """Inference only: post_act(BN_eval(pre_act(conv(x) + bias))) with the eval-mode BatchNorm and the activations
    folded into the epilogue of the MFMA kernels -- no separate normalisation / activation pass over the output.
    bn: None or (gamma, beta, running_mean, running_var, eps).  bf16 1x1 / 32->32 convolutions take the fused kernels; every
    other shape (and the fp32 parity mode) runs convolution, `batchnorm(training=False)` and `act` one after the other."""
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        raise TcctError('conv_bn_act is inference-only (call it under torch.no_grad())')
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    tok = x.dim() == 3
    x4 = x.unsqueeze(2) if tok else x
    w4 = w.view(w.shape[0], w.shape[1], 1, 1) if w.dim() == 2 else w
    _chk(x4, w4, bias)
    N, H, W, Cin = x4.shape
    Cout, Cin_w, KH, KW = w4.shape
    pre, post = ACT[pre_act], ACT[post_act]
    route = conv_route(x4.dtype, x4.dtype, Cin, Cin_w, Cout, KH, KW, stride, ph, pw)
    mfma = route == 'c32'
    pwk = route == 'pw' and (bn is not None or pre != 0 or post != 0)
    if bn is not None and Cin == 32 and route in ('slabs', 'wide33'):
        # round 6: a wider convolution with ONE input slab (MPViT stem[1], 32 -> 64): every 32-channel output slab with its part of the eval-mode BatchNorm + activations
        # in the epilogue (no separate normalisation pass over the 64-channel tensor)
        y = torch.empty((N, H, W, Cout), device=x.device, dtype=x.dtype)
        for oh in range(Cout // 32):
            sl = slice(32 * oh, 32 * oh + 32)
            ab = _eval_ab(bn, 32, x.device, sl)
            wp = torch.empty(KH * KW * 1024, device=x.device, dtype=torch.bfloat16)
            lib.conv32_pack_weights_sub(w4, wp, KH, KW, 0, Cin, 32 * oh, 0)
            lib.conv32_fwd_strided_affine(x4, wp, bias[sl] if bias is not None else None, y, N, H, W, KH, KW, ph, pw, Cin, 0, Cout, 32 * oh, ab, pre, post)
        return y.squeeze(2) if tok else y
    if not (mfma or pwk):
        y = conv2d(x, w, bias, stride, pad)
        if bn is not None:
            return batchnorm(y, bn[0], bn[1], bn[2], bn[3], None, bn[4], 0.1, pre_act, post_act, training=False)
        if pre != 0:
            y = act(y, pre_act)
        return act(y, post_act) if post != 0 else y
    ab = _eval_ab(bn, Cout, x.device) if bn is not None else None
    y = torch.empty((N, H, W, Cout), device=x.device, dtype=x.dtype)
    if pwk:
        lib.pw_fwd_affine(x4, w4, bias, y, N * H * W, Cin, Cout, ab, pre, post, dtype_code(y.dtype))
    else:
        wp = torch.empty(KH * KW * 1024, device=x.device, dtype=torch.bfloat16)
        lib.conv32_pack_weights(w4, wp, KH, KW, 0)
        lib.conv32_fwd_affine(x4, wp, bias, y, N, H, W, KH, KW, ph, pw, ab, pre, post)
    return y.squeeze(2) if tok else y


def _eval_ab(bn, C, device, sl=slice(None)):
    """{a[C], b[C]} of an eval-mode BatchNorm bn = (gamma, beta, running_mean, running_var, eps); sl: the channels of one output slab"""
    ab = torch.empty(2 * C, device=device, dtype=torch.float32)
    lib.bn_eval_ab(C, bn[0][sl], bn[1][sl], float(bn[4]), bn[2][sl], bn[3][sl], torch.empty(2 * C, device=device, dtype=torch.float32), ab)
    return ab


def conv_bn_residual_eval_ok(x, w, bias, stride, pad, pre_act, post_act, residual):
    """inference: residual + BN_eval(conv1x1(x)) as ONE GEMM (tcct_pw_fwd_affine_residual): bf16 rows, square 64 / 96 / 128, no activation"""
    return (INFER_FUSE and not torch.is_grad_enabled() and residual is not None and x.dtype == torch.bfloat16 and x.dim() == 4 and x.is_cuda and stride == 1
            and tuple(pad) == (0, 0) and ACT[pre_act] == 0 and ACT[post_act] == 0 and tuple(w.shape[2:]) == (1, 1) and w.shape[0] == w.shape[1] == x.shape[-1]
            and x.shape[-1] in (64, 96, 128) and residual.shape == x.shape and residual.dtype == x.dtype and x.numel() * 2 < 2 ** 31)


def conv_bn_residual_eval(x, w, bias, bn, residual):
    _chk(x, w, bias, residual)
    C = x.shape[-1]
    y = torch.empty_like(x)
    lib.pw_fwd_affine_residual(x, w, bias, _eval_ab(bn, C, x.device), residual, y, x.numel() // C, C, C)
    return y


def invres_tail_eval_ok(y_dw, w, bias, residual):
    """inference: x + BN(conv2(hswish(BN(y_dw)))) as ONE GEMM (tcct_pw_fwd_xaff_affine_residual)"""
    return (INFER_FUSE and not torch.is_grad_enabled() and y_dw.dtype == torch.bfloat16 and y_dw.dim() == 4 and y_dw.is_cuda and y_dw.shape[-1] in (64, 96, 128)
            and tuple(w.shape) == (y_dw.shape[-1], y_dw.shape[-1], 1, 1) and residual.shape == y_dw.shape and residual.dtype == y_dw.dtype and y_dw.numel() * 2 < 2 ** 31)


def invres_tail_eval(y_dw, bn_norm, w, bias, bn2, residual):
    _chk(y_dw, w, bias, residual)
    C = y_dw.shape[-1]
    out = torch.empty_like(y_dw)
    lib.pw_fwd_xaff_affine_residual(y_dw, _eval_ab(bn_norm, C, y_dw.device), w, bias, _eval_ab(bn2, C, y_dw.device), residual, out, y_dw.numel() // C, C, C)
    return out


def conv1x1_cat2_bn_act_eval_ok(x1, x2, w, post_act):
    """inference: post_act(BN_eval(conv1x1(cat[x1, x2]))) without the concatenation (tcct_pw_fwd_cat2_affine): two 64-channel bf16 tensors, 96 outputs"""
    return (INFER_FUSE and not torch.is_grad_enabled() and x1.dtype == torch.bfloat16 and x1.dim() == 4 and x1.is_cuda and x1.shape[-1] == 64 and x2.shape == x1.shape
            and x2.dtype == x1.dtype and tuple(w.shape) == (96, 128, 1, 1) and x1.numel() * 4 < 2 ** 31)


def conv1x1_cat2_bn_act_eval(x1, x2, w, bn, post_act):
    _chk(x1, x2, w)
    y = torch.empty(x1.shape[:-1] + (96,), device=x1.device, dtype=x1.dtype)
    lib.pw_fwd_cat2_affine(x1, x2, w, None, _eval_ab(bn, 96, x1.device), ACT[post_act], y, x1.numel() // 64, 128, 96)
    return y


def bn2_add_act_eval(xa, bnA, xb, bnB, pre_act='lrelu', act_kind='gelu'):
    """Inference only: act(BN_A(pre(xa)) + BN_B(pre(xb))) with running statistics, one pass (CrossCNNBlock junction).
    bnA/bnB: (gamma, beta, running_mean, running_var, eps)."""
    if torch.is_grad_enabled() and (xa.requires_grad or xb.requires_grad):
        raise TcctError('bn2_add_act_eval is inference-only')
    _chk(xa, xb)
    C = xa.shape[-1]
    M = xa.numel() // C
    abA, abB = _eval_ab(bnA, C, xa.device), _eval_ab(bnB, C, xa.device)
    y = torch.empty_like(xa)
    lib.bn2_add_act_fwd(xa, xb, y, M, C, abA, abB, ACT[pre_act], ACT[act_kind], dtype_code(xa.dtype))
    return y


def _scale_rows(dy, scale):
    """scale[b] * dy[b] (the DropPath scale of a residual branch in its backward); dy itself without a scale"""
    if scale is None:
        return dy
    B = dy.shape[0]
    dz = torch.empty_like(dy)
    lib.scale_rows(dy, scale, dz, B, dy.numel() // B, dtype_code(dy.dtype))
    return dz


def _pw_backward(x, dz, w, wsrc, bsrc):
    """-> (dx, dw, db) of a bf16 pointwise convolution / Linear z = x W^T + bias with a bias: ONE pass over dz (tcct_pw_bwd) where the shape allows, else the
    transposed GEMM plus the weight gradient on the side stream"""
    K, Cout = x.shape[-1], w.shape[0]
    M = x.numel() // K
    dx = torch.empty_like(x)
    if _pw_bwd_ok(x, dz, K, K, Cout, 1, 1, 1, 0, 0):
        dw, db = _grad_out(wsrc, tuple(w.shape)), _grad_out(bsrc)
        lib.pw_bwd(x, dz, w, None, dx, dw, db, M, K, Cout)
        return dx, dw, db
    lib.pw_fwd(dz, w, None, dx, M, Cout, K, 1, dtype_code(x.dtype))
    with _wgrad_stream(_slot_written(wsrc, bsrc), x, dz):
        dw, db = _grad_out(wsrc, tuple(w.shape)), _grad_out(bsrc)
        lib.pw_wgrad(x, dz, dw, db, M, K, Cout)
    return dx, dw, db


def _pw_backward_gelu(x1, dz, w, wsrc, bsrc):
    """-> (dx1, dw, db) of z = gelu(x1) W^T + bias, bf16, from ONE pass over dz with GELU and its derivative applied while the tiles are staged
    (tcct_pw_bwd_gelu): neither h = gelu(x1) nor dh exist in HBM"""
    K, Cout = x1.shape[-1], w.shape[0]
    dx1 = torch.empty_like(x1)
    dw, db = _grad_out(wsrc, tuple(w.shape)), _grad_out(bsrc)
    lib.pw_bwd_gelu(x1, dz, w, dx1, dw, db, x1.numel() // K, K, Cout)
    return dx1, dw, db


def _sum2(ga, gb):
    """the contiguous sum of two optional output gradients of one shape; the one that is there when the other is None; None without either"""
    if ga is None or gb is None:
        g = gb if ga is None else ga
        return None if g is None else _c(g)
    dz = torch.empty_like(gb)
    lib.add(_c(ga), _c(gb), dz, dz.numel(), dtype_code(dz.dtype))
    return dz


MLP_GELU_FUSE = True         # False: GELU as its own pass between fc1 and fc2 (round-3 form; A/B timing)


class _LinearResidual(_FastFunction):
    """res + scale[b] * (x W^T + bias) on tokens [B,N,C] (Mlp.fc2 + DropPath scale + residual add in the GEMM epilogue).
    gelu: res + scale[b] * (gelu(x) W^T + bias) with x the PRE-activation of Mlp.fc1 (reference nets/tcct.py:29-53,468): GELU is applied while the GEMM
    kernels stage their tiles (tcct_pw_fwd_gelu_residual / _pw_backward_gelu), so neither h = gelu(x) nor dh exist in HBM -- bit-identical to
    act(x, 'gelu') followed by the plain form (same formula, same bf16 roundings), two tensor passes fewer forward and three fewer backward."""

    @staticmethod
    def forward(ctx, x, w, bias, res, scale, gelu=False):
        _chk(x, w, bias, res, scale)
        B, Nt, K = x.shape
        Cout = w.shape[0]
        y = torch.empty((B, Nt, Cout), device=x.device, dtype=x.dtype)
        if gelu:
            lib.pw_fwd_gelu_residual(x, w, bias, res, scale, Nt, y, B * Nt, K, Cout)
        else:
            lib.pw_fwd_residual(x, w, bias, res, scale, Nt, y, None, B * Nt, K, Cout)
        ctx.save_for_backward(x, w)
        ctx.scale, ctx.params, ctx.gelu = scale, (w, bias), gelu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        wsrc, bsrc = ctx.params
        dy = _c(dy)
        dx, dw, db = (_pw_backward_gelu if ctx.gelu else _pw_backward)(x, _scale_rows(dy, ctx.scale), w, wsrc, bsrc)
        return dx, _ret(dw, wsrc), _ret(db, bsrc), dy, None, None


class _MlpTail(_FastFunction):
    """t2 = t1 + scale[b] * fc2(gelu(fc1(cur2))) with cur2 = LayerNorm2(t1) as stored by the node in front (ln_metapool_residual_ln): MHCABlock's second half
    (reference nets/tcct.py:466-468) as ONE autograd node, so that its backward can run LayerNorm2's backward in fc1's input-gradient epilogue
    (tcct_pw_bwd_lnb): the gradient of cur2 is never written, the stand-alone LayerNorm backward pass does not run.  The node returns the COMPLETE gradient of
    t1 (residual path + through LayerNorm2) and none for cur2; dgamma2 / dbeta2 come out of the same kernel."""

    @staticmethod
    def forward(ctx, t1, cur2, mr2, g2, b2, w1, bias1, w2, bias2, scale):
        _chk(t1, cur2, mr2, g2, b2, w1, bias1, w2, bias2, scale)
        B, Nt, K = t1.shape
        M = B * Nt
        y1 = torch.empty_like(t1)
        lib.pw_fwd(cur2, w1, bias1, y1, M, K, K, 0, dtype_code(t1.dtype))
        t2 = torch.empty_like(t1)
        lib.pw_fwd_gelu_residual(y1, w2, bias2, t1, scale, Nt, t2, M, K, K)
        ctx.save_for_backward(t1, cur2, mr2, y1, g2, w1, w2)
        ctx.scale = scale
        ctx.params = (g2, b2, w1, bias1, w2, bias2)
        return t2

    @staticmethod
    def backward(ctx, dt2):
        t1, cur2, mr2, y1, g2, w1, w2 = ctx.saved_tensors
        g2p, b2p, w1p, bias1p, w2p, bias2p = ctx.params
        dt2 = _as(dt2, t1.dtype)
        B, Nt, K = t1.shape
        M = B * Nt
        dz = _scale_rows(dt2, ctx.scale)
        w1s = _param_of(w1p)
        w2s = _param_of(w2p)
        dy1, dw2, db2 = _pw_backward_gelu(y1, dz, w2, w2s, bias2p)
        dt1 = torch.empty_like(t1)
        dw1, db1 = _grad_out(w1s, tuple(w1.shape)), _grad_out(bias1p)
        dg2, dbeta2 = _grad_out(g2p), _grad_out(b2p)
        lib.pw_bwd_lnb(cur2, dy1, w1, t1, mr2, g2, dt2, dt1, dw1, db1, dg2, dbeta2, M, K, K)
        return (dt1, None, None, _ret(dg2, g2p), _ret(dbeta2, b2p), _ret(dw1, w1s), _ret(db1, bias1p), _ret(dw2, w2s), _ret(db2, bias2p), None)


MLP_TAIL_FUSE = True      # False: LayerNorm2 keeps its own backward pass (A/B timing)


def mlp_tail_ok(t1, cur2, w1, bias1, w2, bias2):
    return (MLP_TAIL_FUSE and MLP_GELU_FUSE and torch.is_grad_enabled() and t1.dtype == torch.bfloat16 and t1.dim() == 3 and t1.shape[-1] == 64
            and cur2.shape == t1.shape and tuple(w1.shape) == (64, 64) and tuple(w2.shape) == (64, 64) and bias1 is not None and bias2 is not None
            and t1.is_contiguous() and cur2.is_contiguous() and t1.numel() * 2 < 2 ** 31)


def mlp_tail(t1, cur2, mr2, g2, b2, w1, bias1, w2, bias2, scale=None):
    """t1 + scale[b] * fc2(gelu(fc1(cur2))), cur2 = LayerNorm2(t1) with statistics mr2 (from ln_metapool_residual_ln); check mlp_tail_ok first"""
    return _MlpTail.apply(t1, cur2, mr2, g2, b2, w1, bias1, w2, bias2, scale)


def gelu_linear_residual_ok(x1, w, bias, res):
    return (MLP_GELU_FUSE and torch.is_grad_enabled() and x1.dtype == torch.bfloat16 and x1.dim() == 3 and w.dim() == 2
            and x1.shape[-1] in (64, 96) and w.shape[0] == x1.shape[-1] and w.shape[1] == x1.shape[-1] and bias is not None
            and res.shape == x1.shape and x1.numel() * 2 < 2 ** 31)


def gelu_linear_residual(x1, w, bias, res, scale=None):
    """res + scale[b] * Linear(gelu(x1)); check gelu_linear_residual_ok first"""
    return _LinearResidual.apply(x1, w, bias, res, scale, True)


class _Conv1x1AndSum(_FastFunction):
    """(d, d + res) with d = conv1x1(x): both written by one GEMM epilogue (decoder `post` convolution + the `x_i + y_i` that follows)"""

    @staticmethod
    def forward(ctx, x, w, bias, res):
        ctx.set_materialize_grads(False)      # an unused output must arrive as None in backward(), not as a zero-filled tensor
        _chk(x, w, bias, res)
        N_, H, W_, K = x.shape
        Cout = w.shape[0]
        d = torch.empty((N_, H, W_, Cout), device=x.device, dtype=x.dtype)
        s_ = torch.empty_like(d)
        lib.pw_fwd_residual(x, w, bias, res, None, 1, s_, d, N_ * H * W_, K, Cout)
        ctx.save_for_backward(x, w)
        ctx.params = (w, bias)
        return d, s_

    @staticmethod
    def backward(ctx, gd, gs):
        x, w = ctx.saved_tensors
        wsrc, bsrc = ctx.params
        if gd is None and gs is None:
            return None, None, None, None
        dx, dw, db = _pw_backward(x, _sum2(gd, gs), w, wsrc, bsrc)
        return dx, _ret(dw, wsrc), _ret(db, bsrc), (None if gs is None else _c(gs))


class _UpSkipConv(_FastFunction):
    """decoder block tail (MPUpBlock, reference tcct.py:908-914 + the `x_i + y_i` of FTC.forward :1028-1031) as one node:
         u = resize_x2(y) + skip;  d = conv1x1(u);  s = d + skip        -> (d, s)
    One node instead of bilinear + conv1x1_and_sum so that the skip tensor's two gradients (through u and through s) leave the
    input-gradient GEMM already summed (tcct_pw_dgrad_residual) -- autograd would otherwise add them in a separate pass."""

    @staticmethod
    def forward(ctx, y, skip, w, bias, align, want_plain=True):
        ctx.set_materialize_grads(False)      # an unused output must arrive as None in backward(), not as a zero-filled tensor
        _chk(y, skip, w, bias)
        N_, H, W_, C = y.shape
        _, Ho, Wo, _ = skip.shape
        Cout = w.shape[0]
        u = torch.empty_like(skip)
        lib.bilinear_add_fwd(y, skip, u, N_, H, W_, C, Ho, Wo, int(align), dtype_code(y.dtype))
        s_ = torch.empty((N_, Ho, Wo, Cout), device=y.device, dtype=y.dtype)
        # want_plain=False (the LAST decoder block: FTC.forward reads only x_0 + y_0, tcct.py:1031-1035): the 452 MB `d` of the bench shape is never written
        d = torch.empty_like(s_) if want_plain else None
        lib.pw_fwd_residual(u, w, bias, skip, None, 1, s_, d, N_ * Ho * Wo, C, Cout)
        ctx.save_for_backward(u, w)
        ctx.params = (w, bias)
        ctx.cfg = (N_, H, W_, C, Ho, Wo, int(align))
        if d is None:
            d = s_.new_empty(0)
            ctx.mark_non_differentiable(d)
        return d, s_

    @staticmethod
    def backward(ctx, gd, gs):
        u, w = ctx.saved_tensors
        wsrc, bsrc = ctx.params
        N_, H, W_, C, Ho, Wo, align = ctx.cfg
        if gd is None and gs is None:
            return None, None, None, None, None, None
        Cout, M = w.shape[0], N_ * Ho * Wo
        gd, gs = (None if gd is None else _c(gd)), (None if gs is None else _c(gs))
        dw = dz = None
        if gs is None:          # only d was used: the skip tensor's gradient is the one through u
            du, dw, db = _pw_backward(u, gd, w, wsrc, bsrc)
            dskip = du
        else:
            du, dskip = torch.empty_like(u), torch.empty_like(u)
            if gd is not None and C == 32 and Cout == 32 and u.dtype == torch.bfloat16 and _pw_bwd_ok(u, gs, C, C, Cout, 1, 1, 1, 0, 0):
                # the two output gradients are summed while the backward kernel stages its tiles: no add pass
                dw, db = _grad_out(wsrc, tuple(w.shape)), _grad_out(bsrc)
                lib.pw_bwd_residual2_sum(u, gd, gs, w, gs, dskip, du, dw, db, M, C, Cout)
            else:
                dz = _sum2(gd, gs)
                if _pw_bwd_ok(u, dz, C, C, Cout, 1, 1, 1, 0, 0):       # both input gradients and the weight / bias gradients from ONE pass over dz
                    dw, db = _grad_out(wsrc, tuple(w.shape)), _grad_out(bsrc)
                    lib.pw_bwd_residual2(u, dz, w, gs, dskip, du, dw, db, M, C, Cout)
                else:
                    lib.pw_dgrad_residual(dz, w, gs, dskip, du, M, Cout, C)
        dy = torch.empty((N_, H, W_, C), device=u.device, dtype=u.dtype)
        lib.bilinear_bwd(du, dy, N_, H, W_, C, Ho, Wo, align, dtype_code(u.dtype))
        if dw is None:
            with _wgrad_stream(_slot_written(wsrc, bsrc), u, dz):
                dw, db = _grad_out(wsrc, tuple(w.shape)), _grad_out(bsrc)
                lib.pw_wgrad(u, dz, dw, db, M, C, Cout)
        return dy, dskip, _ret(dw, wsrc), _ret(db, bsrc), None, None


def up_skip_conv(y, skip, w, bias, align_corners=True, want_plain=True):
    """(d, d + skip) with d = conv1x1(resize(y -> skip's size) + skip); the fused node needs bf16 with square 1x1 weights.
    want_plain=False: d is not needed (returned as None)"""
    ok = (y.dtype == torch.bfloat16 and skip.dtype == y.dtype and y.dim() == 4 and y.shape[-1] % 32 == 0 and y.shape[-1] <= 160
          and w.shape[0] == y.shape[-1] and w.shape[1] == y.shape[-1] and tuple(w.shape[2:]) == (1, 1) and bias is not None
          and skip.shape[-1] == y.shape[-1] and tuple(skip.shape[1:3]) != tuple(y.shape[1:3]) and torch.is_grad_enabled())
    if not ok:
        return conv1x1_and_sum(bilinear(y, tuple(skip.shape[1:3]), align_corners, residual=skip), w, bias, skip)
    d, s_ = _UpSkipConv.apply(y, skip, w, bias, bool(align_corners), bool(want_plain))
    return (d if want_plain else None), s_


TAIL_COMPOSE = True      # False: resize + add, post convolution (+ sum), t324 as three kernels (round-3 form; A/B timing)


def _resize_to(y, skip, align):
    """v = y resized to the height and width of skip (bilinear, tcct_bilinear_fwd)"""
    N_, H, W_, C = y.shape
    v = torch.empty_like(skip)
    lib.bilinear_fwd(y, v, N_, H, W_, C, skip.shape[1], skip.shape[2], int(align), dtype_code(y.dtype))
    return v


def _tail_g0(v, skip, w1, b1, w2, b2):
    """-> (g0, wc): g0 = t32(post(v + skip) + skip) as ONE 64 -> 32 GEMM over the never-materialised [v | skip] with the composed weight wc [32, 64]
    (tcct_tail_compose)"""
    wc = torch.empty((32, 64), device=v.device, dtype=torch.float32)
    c = torch.empty(32, device=v.device, dtype=torch.float32)
    lib.tail_compose(w1, b1, w2, b2, wc, c)
    g = torch.empty_like(skip)
    lib.pw_fwd_cat2(v, skip, 32, wc, c, g, v.numel() // 32, 64, 32, None, 0)
    return g, wc


def _tail_compose3(w1, b1, w2, b2, w3, b3, pad8=False):
    """the composed weights of aux(t32(post(v + skip) + skip)) (tcct_tail_compose3) -> (wcc [nc, 64] over [v | skip], its halves wa and wb [nc, 32, 1, 1],
    the bias ccc [nc], wa8).  pad8: wa is the first nc rows of wa8 [8, 32, 1, 1], whose other rows are zero; else wa8 is None"""
    nc, f32 = w3.shape[0], dict(device=w3.device, dtype=torch.float32)
    wcc = torch.empty((nc, 64), **f32)
    wa8 = torch.zeros((8, 32, 1, 1), **f32) if pad8 else None
    wa, wb = (wa8[:nc] if pad8 else torch.empty((nc, 32, 1, 1), **f32)), torch.empty((nc, 32, 1, 1), **f32)
    ccc = torch.empty(nc, **f32)
    lib.tail_compose3(w1, b1, w2, b2, w3, b3, nc, wcc, wa, wb, ccc)
    return wcc, wa, wb, ccc, wa8


def _composed_wgrad(pairs, params, decompose, keep):
    """The parameter gradients of a composed head, on the weight-gradient stream: per (x, g, rows, wants_bias) of `pairs` the small-N sum g^T x [nc, 32]
    into a zeroed buffer (the one with wants_bias also sums g into the composed bias' gradient), then decompose(nc, sums..., bias sum, *destinations of
    params).  keep: every tensor the side stream reads, kept alive until it is joined.  -> what backward returns for params, in their order"""
    nc, dev = pairs[0][1].shape[-1], pairs[0][0].device
    F32_, BF_ = dtype_code(torch.float32), dtype_code(pairs[0][0].dtype)
    with _wgrad_stream(_slot_written(*params), *keep):
        sums = [ZERO.get((nc, 32), torch.float32, dev) for _ in pairs]
        dbias = ZERO.get((nc,), torch.float32, dev)
        for (x, g, rows, wants_bias), dw in zip(pairs, sums):
            lib.pw_wgrad_smalln(x, g, dw, dbias if wants_bias else None, rows, 32, nc, BF_, F32_)
        outs = [_grad_out(p, tuple(p.shape)) for p in params]
        decompose(nc, *sums, dbias, *outs)
    return tuple(_ret(o, p) for o, p in zip(outs, params))


class _UpSkipConvT32(_FastFunction):
    """g0 = t32(post(up(y) + skip) + skip) for the LAST decoder block (reference nets/tcct.py:908-914, :1031, :1035-1040) as ONE 64 -> 32 GEMM over the
    never-materialised concatenation [up(y) | skip] with composed weights (csrc/decoder_tail.hip): u, d0 and s0 are not written, the backward pass is
    one fused kernel + a 32 x 32 de-composition of the weight gradients."""

    @staticmethod
    def forward(ctx, y, skip, w1, b1, w2, b2, align):
        _chk(y, skip, w1, b1, w2, b2)
        N_, H, W_, C = y.shape
        _, Ho, Wo, _ = skip.shape
        v = _resize_to(y, skip, align)
        g, wc = _tail_g0(v, skip, w1, b1, w2, b2)
        ctx.save_for_backward(v, skip, wc)
        ctx.params = (w1, b1, w2, b2)
        ctx.cfg = (N_, H, W_, C, Ho, Wo, int(align))
        return g

    @staticmethod
    def backward(ctx, dg):
        v, skip, wc = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        N_, H, W_, C, Ho, Wo, align = ctx.cfg
        dg = _as(dg, v.dtype)
        dev = v.device
        M = N_ * Ho * Wo
        dv, dskip = torch.empty_like(v), torch.empty_like(skip)
        dwc = ZERO.get((32, 64), torch.float32, dev)
        dc = ZERO.get((32,), torch.float32, dev)
        lib.pw_bwd_cat2_bias(v, skip, dg, wc, dv, dskip, dwc, dc, M, 64, 32)
        dy = torch.empty((N_, H, W_, C), device=dev, dtype=v.dtype)
        lib.bilinear_bwd(dv, dy, N_, H, W_, C, Ho, Wo, align, dtype_code(v.dtype))
        dw1, db1, dw2, db2 = _grad_out(w1, tuple(w1.shape)), _grad_out(b1), _grad_out(w2, tuple(w2.shape)), _grad_out(b2)
        lib.tail_compose_bwd(w1, b1, w2, dwc, dc, dw1, db1, dw2, db2)
        return dy, dskip, _ret(dw1, w1), _ret(db1, b1), _ret(dw2, w2), _ret(db2, b2), None


def up_skip_conv_t32_ok(y, skip, w1, b1, w2, b2):
    return (TAIL_COMPOSE and y.dtype == torch.bfloat16 and skip.dtype == y.dtype and y.dim() == 4       # (the caller requires a train-mode block)
            and y.shape[-1] == 32 and skip.shape[-1] == 32 and tuple(skip.shape[1:3]) == (2 * y.shape[1], 2 * y.shape[2])
            and tuple(w1.shape) == (32, 32, 1, 1) and tuple(w2.shape) == (32, 32, 1, 1) and b1 is not None and b2 is not None
            and w1.is_contiguous() and w2.is_contiguous() and skip.numel() * 2 < 2 ** 31)


def up_skip_conv_t32(y, skip, w1, b1, w2, b2, align_corners=True):
    """t32(post(resize_x2(y) + skip) + skip) with post = (w1, b1), t32 = (w2, b2), both 1x1 32 -> 32; check up_skip_conv_t32_ok first"""
    return _UpSkipConvT32.apply(y, skip, w1, b1, w2, b2, bool(align_corners))


class _UpSkipConvT32Aux(_FastFunction):
    """logits0 = aux0(t32(post(up(y) + skip) + skip)) (reference nets/tcct.py:908-914,1031,1035-1041) as ONE 64 -> n_class GEMM with fp32 output over
    [up(y) | skip] (csrc/decoder_tail.hip, `compose3`): for steps in which nothing else reads g0 -- the feature-polarization loss is off.  g0 and dg0
    never exist; the backward pass uses the small-N kernels of the aux heads on the two halves.  Returns (logits, v): v = up(y) (no gradient) lets
    `FTC.feats` rebuild g0 on demand."""

    @staticmethod
    def forward(ctx, y, skip, w1, b1, w2, b2, w3, b3, align):
        _chk(y, skip, w1, b1, w2, b2, w3, b3)
        N_, H, W_, C = y.shape
        _, Ho, Wo, _ = skip.shape
        dev, nc = y.device, w3.shape[0]
        v = _resize_to(y, skip, align)
        wcc, wa, wb, ccc, _ = _tail_compose3(w1, b1, w2, b2, w3, b3)
        lg = torch.empty((N_, Ho, Wo, nc), device=dev, dtype=torch.float32)
        lib.pw_fwd_cat2_f32(v, skip, 32, wcc, ccc, lg, N_ * Ho * Wo, 64, nc)
        ctx.save_for_backward(v, skip, wa, wb)
        ctx.params = (w1, b1, w2, b2, w3, b3)
        ctx.cfg = (N_, H, W_, C, Ho, Wo, int(align), nc)
        ctx.mark_non_differentiable(v)
        return lg, v

    @staticmethod
    def backward(ctx, dl, _dv):
        v, skip, wa, wb = ctx.saved_tensors
        w1, b1, w2, b2, w3, b3 = ctx.params
        N_, H, W_, C, Ho, Wo, align, nc = ctx.cfg
        dl = _as(dl, torch.float32)
        dev = v.device
        M = N_ * Ho * Wo
        dv, dskip = torch.empty_like(v), torch.empty_like(skip)
        F32_, BF_ = dtype_code(torch.float32), dtype_code(v.dtype)
        lib.conv2d_dgrad(dl, wa, dv, N_, Ho, Wo, 32, nc, 1, 1, 0, 0, F32_, BF_)
        lib.conv2d_dgrad(dl, wb, dskip, N_, Ho, Wo, 32, nc, 1, 1, 0, 0, F32_, BF_)
        dy = torch.empty((N_, H, W_, C), device=dev, dtype=v.dtype)
        lib.bilinear_bwd(dv, dy, N_, H, W_, C, Ho, Wo, align, BF_)
        dparams = _composed_wgrad([(v, dl, M, True), (skip, dl, M, False)], ctx.params, lambda *a: lib.tail_compose3_bwd(w1, b1, w2, b2, w3, *a),
                                  keep=(v, skip, dl, wa, wb))
        return (dy, dskip) + dparams + (None,)


class _UpSkipConvT32AuxLow(_FastFunction):
    """The same logits0 = aux0(t32(post(up(y) + skip) + skip)) with the resize COMMUTED behind the 1x1 convolution (round 4): bilinear interpolation is linear
    and acts per channel, so  W up(y) = up(W y):
        logits0 = up(Wa y) + Wb skip + c,      Wa = W3 W2 W1 [C x 32] applied at the LOW resolution,  Wb = W3 (W2 W1 + W2),  c = W3 (W2 b1 + b2) + b3
    z = Wa y is n_class channels at a quarter of the pixels (fp32); the resized 32-channel tensor v = up(y) (452 MB at the bench shape) is never written or
    read, and neither is its gradient: backward = bilinear^T on n_class channels, two small-N input-gradient kernels, two small-N weight-gradient
    kernels (one of them at the low resolution) and the de-composition of `compose3`."""

    @staticmethod
    def forward(ctx, y, skip, w1, b1, w2, b2, w3, b3, align):
        _chk(y, skip, w1, b1, w2, b2, w3, b3)
        N_, H, W_, C = y.shape
        _, Ho, Wo, _ = skip.shape
        dev, nc = y.device, w3.shape[0]
        F32_ = dtype_code(torch.float32)
        # wa8: rows >= n_class stay zero: the low-resolution product has 8 channels (16-byte taps)
        wcc, wa, wb, ccc, wa8 = _tail_compose3(w1, b1, w2, b2, w3, b3, pad8=True)
        lg = torch.empty((N_, Ho, Wo, nc), device=dev, dtype=torch.float32)
        if HEAD_UPADD and align and Ho == 2 * H and Wo == 2 * W_:
            z8 = torch.empty((N_, H, W_, 8), device=dev, dtype=torch.float32)
            lib.pw_fwd(y, wa8, None, z8, N_ * H * W_, 32, 8, 0, F32_)
            lib.pw_fwd_f32_upadd(skip, wb, ccc, lg, N_, H, W_, 32, nc, z8)             # up(z) added in the epilogue of the full-resolution GEMM
        else:
            z = torch.empty((N_, H, W_, nc), device=dev, dtype=torch.float32)
            lib.pw_fwd(y, wa, None, z, N_ * H * W_, 32, nc, 0, F32_)
            lib.pw_fwd(skip, wb, ccc, lg, N_ * Ho * Wo, 32, nc, 0, F32_)
            lib.bilinear_add_fwd(z, lg, lg, N_, H, W_, nc, Ho, Wo, int(align), F32_)   # in place: every element reads its own addend, then is written
        ctx.save_for_backward(y, skip, wa, wb)
        ctx.params = (w1, b1, w2, b2, w3, b3)
        ctx.cfg = (N_, H, W_, C, Ho, Wo, int(align), nc)
        # skip is the full-size output of a BatchNorm + pool node whose backward kernels can form Wb^T dl themselves (SKIP0_LOWRANK below)
        link = getattr(skip, '_skip0', None) if SKIP0_LOWRANK else None
        ctx.skip0 = link if (link is not None and link.ok and 2 <= nc <= 8 and ctx.needs_input_grad[1] and not grad_is_watched(skip)) else None
        if ctx.skip0 is not None:
            del link.recipes[:]         # a recipe an earlier backward pass filed and never delivered (it raised before the producer's node ran) must not be added to this one's
        return lg

    @staticmethod
    def backward(ctx, dl):
        y, skip, wa, wb = ctx.saved_tensors
        N_, H, W_, C, Ho, Wo, align, nc = ctx.cfg
        dl = _as(dl, torch.float32)
        dev = y.device
        F32_, BF_ = dtype_code(torch.float32), dtype_code(y.dtype)
        dz = torch.empty((N_, H, W_, nc), device=dev, dtype=torch.float32)
        lib.bilinear_bwd(dl, dz, N_, H, W_, nc, Ho, Wo, align, F32_)
        dy = torch.empty_like(y)
        lib.conv2d_dgrad(dz, wa, dy, N_, H, W_, 32, nc, 1, 1, 0, 0, F32_, BF_)
        if ctx.skip0 is not None:
            # d loss / d skip = Wb^T dl has rank n_class: the producer's backward kernels form it on load from (dl, wb); autograd carries the placeholder
            dskip = ctx.skip0.file((dl, wb, nc), skip.shape, skip.dtype, dev)
        else:
            dskip = torch.empty_like(skip)
            lib.conv2d_dgrad(dl, wb, dskip, N_, Ho, Wo, 32, nc, 1, 1, 0, 0, F32_, BF_)
        dparams = _composed_wgrad([(y, dz, N_ * H * W_, False), (skip, dl, N_ * Ho * Wo, True)], ctx.params,
                                  lambda *a: lib.tail_compose3_bwd(*ctx.params[:5], *a), keep=(y, skip, dl, dz, wa, wb))
        return (dy, dskip) + dparams + (None,)


HEAD_UPADD = True       # False: the resized low-resolution product is added by its own pass (A/B timing)
TAIL_AUX_LOW = True   # False: the composed head reads the resized 32-channel tensor (the first round-4 form; A/B timing)
# True: the composed head hands the gradient of its skip input to the BatchNorm + pool node that produced it as (dl, Wb) and that node's two backward kernels
# form Wb^T dl on load (tcct_bn_pool_bwd_lowrank): the conv2d_dgrad launch and the 32-channel gradient it wrote are gone.  False: the dense tensor (A/B timing)
SKIP0_LOWRANK = True


def up_skip_conv_t32_aux_low(y, skip, w1, b1, w2, b2, w3, b3, align_corners=True):
    """aux(t32(post(resize_x2(y) + skip) + skip)) as fp32 NHWC logits, the resize taken of the n_class-channel product; check up_skip_conv_t32_aux_ok first"""
    return _UpSkipConvT32AuxLow.apply(y, skip, w1, b1, w2, b2, w3, b3, bool(align_corners))


def up_skip_conv_t32_from_y(y, skip, w1, b1, w2, b2, align_corners=True):
    """g0 of the composed tail from the un-resized y (no gradient): what `FTC.feats` needs when the step itself never resized y"""
    with torch.no_grad():
        return _tail_g0(_resize_to(y, skip, align_corners), skip, w1, b1, w2, b2)[0]


TAIL_AUX = True       # False: the composed tail stops at g0, aux0 stays its own kernels (A/B timing)


def up_skip_conv_t32_aux_ok(y, skip, w1, b1, w2, b2, w3, b3):
    return (TAIL_AUX and up_skip_conv_t32_ok(y, skip, w1, b1, w2, b2) and w3.dim() == 4 and tuple(w3.shape[1:]) == (32, 1, 1) and 2 <= w3.shape[0] <= 8
            and b3 is not None and w3.is_contiguous())


def up_skip_conv_t32_aux(y, skip, w1, b1, w2, b2, w3, b3, align_corners=True):
    """(aux(t32(post(resize_x2(y) + skip) + skip)) as fp32 NHWC logits, resize_x2(y)); check up_skip_conv_t32_aux_ok first"""
    return _UpSkipConvT32Aux.apply(y, skip, w1, b1, w2, b2, w3, b3, bool(align_corners))


def up_skip_conv_t32_from_v(v, skip, w1, b1, w2, b2):
    """g0 of the composed tail from an already resized v (no gradient): what `FTC.feats` needs when the step itself skipped g0"""
    with torch.no_grad():
        return _tail_g0(v, skip, w1, b1, w2, b2)[0]


class _HeadThroughT32(_FastFunction):
    """logits_i = aux_i(t32x(s_i)) (reference nets/tcct.py:1036-1044, levels 1-3) as ONE 32 -> n_class GEMM with fp32 output and the composed weight
    Wa Wt (csrc/decoder_tail.hip, `head_compose`): for steps in which nothing else reads g_i = t32x(s_i) -- the feature-polarization loss is off.
    g_i and its gradient never exist; the backward pass runs the aux head's small-N kernels with the composed weight and de-composes the gradients."""

    @staticmethod
    def forward(ctx, s, wt, bt, wa, ba):
        _chk(s, wt, bt, wa, ba)
        N_, H, W_, _ = s.shape
        dev, nc = s.device, wa.shape[0]
        wh = torch.empty((nc, 32, 1, 1), device=dev, dtype=torch.float32)
        ch = torch.empty(nc, device=dev, dtype=torch.float32)
        lib.head_compose(wt, bt, wa, ba, nc, wh, ch)
        lg = torch.empty((N_, H, W_, nc), device=dev, dtype=torch.float32)
        lib.pw_fwd(s, wh, ch, lg, N_ * H * W_, 32, nc, 0, dtype_code(torch.float32))
        ctx.save_for_backward(s, wh)
        ctx.params = (wt, bt, wa, ba)
        return lg

    @staticmethod
    def backward(ctx, dl):
        s, wh = ctx.saved_tensors
        wt, bt, wa, ba = ctx.params
        N_, H, W_, _ = s.shape
        nc = wa.shape[0]
        dl = _as(dl, torch.float32)
        F32_, BF_ = dtype_code(torch.float32), dtype_code(s.dtype)
        ds = torch.empty_like(s)
        lib.conv2d_dgrad(dl, wh, ds, N_, H, W_, 32, nc, 1, 1, 0, 0, F32_, BF_)
        return (ds,) + _composed_wgrad([(s, dl, N_ * H * W_, True)], ctx.params, lambda *a: lib.head_compose_bwd(wt, bt, wa, *a), keep=(s, dl, wh))


HEAD_COMPOSE = True       # False: t32x and aux_i stay two convolutions at levels 1-3 (A/B timing)


def head_through_t32_ok(s, wt, bt, wa, ba):
    return (HEAD_COMPOSE and s.dtype == torch.bfloat16 and s.dim() == 4 and s.shape[-1] == 32 and s.is_contiguous() and tuple(wt.shape) == (32, 32, 1, 1)
            and bt is not None and wa.dim() == 4 and tuple(wa.shape[1:]) == (32, 1, 1) and 2 <= wa.shape[0] <= 8 and ba is not None
            and wt.is_contiguous() and wa.is_contiguous() and s.numel() // 32 < 2 ** 31)


def head_through_t32(s, wt, bt, wa, ba):
    """aux(t32(s)) as fp32 NHWC logits from one GEMM with the composed weight; check head_through_t32_ok first"""
    return _HeadThroughT32.apply(s, wt, bt, wa, ba)


def conv1x1_and_sum(x, w, bias, res):
    """(conv1x1(x), conv1x1(x) + res); bf16 NHWC with channel counts multiples of 32 takes the double-store epilogue"""
    ok = (x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[-1] % 32 == 0 and w.shape[0] % 32 == 0 and w.shape[0] <= 160
          and tuple(w.shape[2:]) == (1, 1) and w.shape[1] == x.shape[-1] and bias is not None and res.shape == x.shape[:-1] + (w.shape[0],)
          and res.dtype == x.dtype)
    if not ok:
        d = conv2d(x, w, bias)
        return d, add(res, d)
    return _Conv1x1AndSum.apply(x, w, bias, res)


def linear_residual(x, w, bias, res, scale=None):
    """res + scale[b] * Linear(x) for token tensors [B,N,C]; bf16 with C multiples of 32 takes the fused epilogue"""
    ok = (x.dtype == torch.bfloat16 and x.dim() == 3 and w.dim() == 2 and x.shape[-1] % 32 == 0 and w.shape[0] % 32 == 0
          and w.shape[0] <= 160 and bias is not None and res.shape == x.shape[:-1] + (w.shape[0],))
    if not ok:
        return residual(res, conv2d(x, w, bias), scale)
    return _LinearResidual.apply(x, w, bias, res, scale, False)


class _PwCat2(_FastFunction):
    """1x1 convolution over the channel concatenation [a | b] without materialising it (MHCA_stage.aggregate)"""

    @staticmethod
    def forward(ctx, a, b, w, stats_box):
        _chk(a, b, w)
        N_, H, W_, Ca = a.shape
        Cb = b.shape[-1]
        Cout = w.shape[0]
        M = N_ * H * W_
        y = torch.empty((N_, H, W_, Cout), device=a.device, dtype=a.dtype)
        sums = None
        if stats_box is not None and Cout % 32 == 0 and Cout <= 128:
            sums = _zeros((2 * Cout,), torch.float64, a.device)
            stats_box[1] = sums
        lib.pw_fwd_cat2(a, b, Ca, w, None, y, M, Ca + Cb, Cout, sums, stats_box[0] if sums is not None else 0)
        ctx.save_for_backward(a, b, w)
        wsrc = _param_of(w)
        ctx.wsrc = wsrc
        return y

    @staticmethod
    def backward(ctx, dy):
        a, b, w = ctx.saved_tensors
        dy = _c(dy)
        N_, H, W_, Ca = a.shape
        Cb, Cout, M = b.shape[-1], w.shape[0], N_ * H * W_
        da, db_ = torch.empty_like(a), torch.empty_like(b)
        if (Ca == 64 and Cb == 64 and Cout % 32 == 0 and Cout <= 128 and dy.dtype == torch.bfloat16
                and a.numel() * 2 < 2 ** 31 and dy.numel() * 2 < 2 ** 31):
            dw = _grad_out(ctx.wsrc, tuple(w.shape))
            lib.pw_bwd_cat2(a, b, dy, w, da, db_, dw, M, Ca + Cb, Cout)
            return da, db_, _ret(dw, ctx.wsrc), None
        lib.pw_dgrad_split2(dy, w, da, db_, Ca, M, Cout, Ca + Cb)
        with _wgrad_stream(_slot_written(ctx.wsrc), a, b, dy):
            dw = _grad_out(ctx.wsrc, tuple(w.shape))
            lib.pw_wgrad_cat2(a, b, Ca, dy, dw, None, M, Ca + Cb, Cout)
        return da, db_, _ret(dw, ctx.wsrc), None


def conv1x1_cat2(a, b, w, stats_pre=None):
    """conv1x1(cat([a, b], channel)) with weight w [Cout, Ca+Cb, 1, 1] (no bias): forward, both input gradients and the weight gradient
    read / write the two halves in place -- no concat / split passes.  bf16 with Ca, Cb multiples of 32 and Cout <= 160; any other
    case takes concat2 + conv2d."""
    Ca, Cb, Cout = a.shape[-1], b.shape[-1], w.shape[0]
    ok = (a.dtype == torch.bfloat16 and b.dtype == a.dtype and a.shape[:-1] == b.shape[:-1] and Ca % 32 == 0 and Cb % 32 == 0
          and Cout % 32 == 0 and Cout <= 160 and tuple(w.shape[1:]) == (Ca + Cb, 1, 1) and a.dim() == 4)
    if not ok:
        return conv2d(concat2(a, b), w, None, stats_pre=stats_pre)
    box = _stats_box(stats_pre)
    return _tag_bn_sums(_PwCat2.apply(a, b, w, box), box)


def im2col3x3_c3(x4, stride=1):
    """x4 NHWC [N,H,W,4] (3 image channels + zero pad) -> 3x3 patch pixels [N,Ho,Wo,32]; no gradient (the image needs none)"""
    _chk(x4)
    N, H, W, C = x4.shape
    if C != 4:
        raise TcctError('im2col3x3_c3 expects the 4-channel NHWC image')
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((N, Ho, Wo, 32), device=x4.device, dtype=x4.dtype)
    lib.im2col3x3_c3(x4.detach(), out, N, H, W, stride, dtype_code(x4.dtype))
    return out


C3_DIRECT = True       # False: im2col + pointwise GEMM for the 3-channel first layers (A/B timing)


class _ConvC3(_FastFunction):
    """cnn.0 / stem.0 (reference nets/tcct.py:873, :674-681): 3 -> 32 channels, 3x3, pad 1, stride 1 / 2, straight from the 4-channel image
    (tcct_c3_fwd / tcct_c3_wgrad): the patch rows are gathered inside the MFMA kernels, the 32-channel im2col tensor (452 MB at the bench
    shape, written once and read twice) does not exist.  The image gets no gradient."""

    @staticmethod
    def forward(ctx, x4, w, bias, stride, stats_box):
        _chk(x4, w, bias)
        B, H, W, _ = x4.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty((B, Ho, Wo, 32), device=x4.device, dtype=torch.bfloat16)
        sums = None
        if stats_box is not None:
            sums = _zeros((64,), torch.float64, x4.device)
            stats_box[1] = sums
        lib.c3_fwd(x4, w, bias, y, B, H, W, stride, sums, stats_box[0] if stats_box is not None else 0, None, 0, 0)
        ctx.save_for_backward(x4)
        ctx.cfg = (stride, w, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        x4, = ctx.saved_tensors
        stride, w, bias = ctx.cfg
        dy = _c(dy)
        B, H, W, _ = x4.shape
        with _wgrad_stream(_slot_written(w, bias), x4, dy):
            dw = _grad_out(w, tuple(w.shape))
            db = _grad_out(bias) if bias is not None else None
            lib.c3_wgrad(x4, dy, dw, db, B, H, W, stride)
        return None, _ret(dw, w), _ret(db, bias), None, None


def _c3_direct_ok(x4, w):
    B, H, W, C = x4.shape
    return (C3_DIRECT and x4.dtype == torch.bfloat16 and C == 4 and tuple(w.shape) == (32, 3, 3, 3) and w.dtype == torch.float32
            and w.is_contiguous() and B * H * W * 64 < 2 ** 31)         # 32-bit byte offsets into the image and into the 32-channel output


def conv3x3_c3(x4, w, bias, stride=1, stats_pre=None, infer_bn=None, post_act=None):
    """3-channel 3x3 conv (pad 1).  bf16, 32 output channels: the direct kernels (_ConvC3).  Otherwise (fp32 parity mode, other widths)
    im2col + 32->32 pointwise GEMM: w [32,3,3,3] is re-laid out to [32, 27->32] by view ops
    (differentiable plumbing on 864 elements), so forward and weight gradient both run on the MFMA pointwise kernels.
    infer_bn (inference only): eval-mode BatchNorm tuple folded, with post_act, into the GEMM epilogue (see conv_bn_act)."""
    if _c3_direct_ok(x4, w):
        _chk(x4)
        if infer_bn is not None:
            if torch.is_grad_enabled() and w.requires_grad:
                raise TcctError('conv3x3_c3(infer_bn=...) is inference-only (call it under torch.no_grad())')
            B, H, W, _ = x4.shape
            ab = _eval_ab(infer_bn, 32, x4.device)
            y = torch.empty((B, (H - 1) // stride + 1, (W - 1) // stride + 1, 32), device=x4.device, dtype=torch.bfloat16)
            if C3_BN_FUSE and ACT[post_act] in (0, ACT['hswish']):      # round 6: the recompute kernel's normalising pass with the eval coefficients (0.10 vs 0.28 ms at level 0)
                lib.c3_bn_fwd_eval(x4, w, bias, y, B, H, W, stride, ab, ACT[post_act])
            else:
                lib.c3_fwd(x4, w, bias, y, B, H, W, stride, None, 0, ab, 0, ACT[post_act])
            return y
        box = _stats_box(stats_pre)
        return _tag_bn_sums(_ConvC3.apply(x4, w, bias, stride, box), box)
    w2 = torch.nn.functional.pad(w.permute(0, 2, 3, 1).reshape(w.shape[0], 27), (0, 5)).contiguous()
    if infer_bn is not None:
        return conv_bn_act(im2col3x3_c3(x4, stride), w2.view(w.shape[0], 32, 1, 1), bias, bn=infer_bn, post_act=post_act)
    return conv2d(im2col3x3_c3(x4, stride), w2.view(w.shape[0], 32, 1, 1), bias, stats_pre=stats_pre)


C3_BN_FUSE = True       # False: convolution (+ statistics) and BatchNorm as separate nodes, the round-3 form (A/B timing)


class _ConvC3BN(_FastFunction):
    """z = post(BN_train(conv3x3(x4) + bias)) for the two 3-channel first layers as ONE node whose convolution output is never stored
    (csrc/c3_bn.hip; reference nets/tcct.py:873 `cnn.0 -> cnn.1`, :55-97 + :674-681 `stem[0]`): the input is the 4-channel image, 1/8 of the
    bytes of the 32-channel output, so forward (statistics pass, normalising pass) and backward (reduction, weight gradient) recompute y on the
    matrix pipes instead of writing it once and reading it three times."""

    @staticmethod
    def forward(ctx, x4, w, bias, gamma, beta, rm, rv, nbt, eps, momentum, stride, post):
        _chk(x4, w, bias, gamma, beta)
        B, H, W, _ = x4.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        z = torch.empty((B, Ho, Wo, 32), device=x4.device, dtype=torch.bfloat16)
        sums = _zeros((64,), torch.float64, x4.device)
        mean_rstd, ab = _bn_coef_bufs(32, x4.device)
        lib.c3_bn_fwd_train(x4, w, bias, z, B, H, W, stride, sums, gamma, beta, eps, momentum, rm, rv, nbt, mean_rstd, ab, post)
        ctx.save_for_backward(x4, mean_rstd, ab)
        ctx.cfg = (stride, post, w, bias, gamma, beta)
        return z

    @staticmethod
    def backward(ctx, dz):
        x4, mean_rstd, ab = ctx.saved_tensors
        stride, post, w, bias, gamma, beta = ctx.cfg
        dz = _as(dz, torch.bfloat16)
        B, H, W, _ = x4.shape
        M = dz.numel() // 32
        dev = x4.device
        raw = _zeros((64,), torch.float64, dev)
        coef = torch.empty(160, device=dev, dtype=torch.float32)
        # nothing downstream waits for this node (the image has no gradient): all of it runs beside the other encoder's tail on the weight-gradient stream
        with _wgrad_stream(_slot_written(w, bias, gamma, beta), x4, dz, coef, mean_rstd, ab):
            dg, db_ = _written_grad_out(gamma, 32), _written_grad_out(beta, 32)
            dw = _grad_out(w, tuple(w.shape))
            dbias = _grad_out(bias) if bias is not None else None
            if C3_ONEPASS:      # reduction and weight gradient from ONE pass over dz (the BatchNorm backward is linear in per-pixel quantities)
                if C3_BWD_FORM != _C3_FORM_SET[0]:
                    lib.c3_bn_bwd_prefetch(C3_BWD_FORM)
                    _C3_FORM_SET[0] = C3_BWD_FORM
                work = _zeros((4160,), torch.float32, dev)
                s96 = _zeros((96,), torch.float64, dev)
                lib.c3_bn_bwd_onepass(x4, w, bias, dz, B, H, W, stride, mean_rstd, ab, work, s96, dw, dbias, dg, db_, post)
            else:
                lib.c3_bn_bwd_reduce(x4, w, bias, dz, B, H, W, stride, ab, raw, post)
                lib.bn_bwd_coef(raw, 1, M, 32, mean_rstd, ab, coef, dg, db_)
                lib.c3_bn_bwd_wgrad(x4, w, bias, dz, B, H, W, stride, coef, dw, dbias, post)
        return None, _ret(dw, w), _ret(dbias, bias), _ret(dg, gamma), _ret(db_, beta), None, None, None, None, None, None, None


C3_BWD_FORM = 4        # kernel form of the one-pass backward (tcct_c3_bn_bwd_prefetch): 4 = wave-private 32-pixel tiles (round 6), 1 = block tiles of 128 pixels (A/B timing)
_C3_FORM_SET = [4]
C3_ONEPASS = True      # False: BatchNorm reduction and weight gradient of the first layers as two passes over dz (A/B timing)


def conv3x3_c3_bn_ok(x4, w, bn_training, post_act):
    # (train-mode BatchNorm, with or without autograd: a no_grad train-mode forward must round where the training step does)
    return (C3_BN_FUSE and bn_training and _c3_direct_ok(x4, w) and ACT[post_act] in (0, ACT['hswish']))


def conv3x3_c3_bn(x4, w, bias, bn, stride=1, post_act=None):
    """post_act(BN_train(conv3x3_c3(x4))); bn = (gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum); check
    conv3x3_c3_bn_ok first"""
    gamma, beta, rm, rv, nbt, eps, mom = bn
    return _ConvC3BN.apply(x4, w, bias, gamma, beta, rm, rv, nbt, float(eps), float(mom), int(stride), ACT[post_act])


class _DwConv(_FastFunction):
    @staticmethod
    def forward(ctx, x, w, bias, stride, add_input, fork=False, stats_box=None, xab=None, xlink=None):
        """fork: also return an alias of x for its other consumers; their gradient is added inside the input-gradient kernel.
        stats_box (_stats_box('none')): the kernel also accumulates the statistics of the train-mode BatchNorm that consumes the output.
        xab (round 4): x is y_prev, the input of a train-mode BatchNorm + Hardswish in front whose normalisation pass was not run (xab = its {a[C], b[C]});
        the kernels apply z = hswish(a y_prev + b) as rows enter their register window.  The gradient returned for x is the gradient of that z."""
        ctx.set_materialize_grads(False)      # an unused output must arrive as None in backward(), not as a zero-filled tensor
        _chk(x, w, bias)
        N, H, W, C = x.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty((N, Ho, Wo, C), device=x.device, dtype=x.dtype)
        ctx.xab = xab
        ctx.xlink = xlink       # the BnLink of the BatchNorm pending on x: the input-gradient kernel delivers its backward sums through it
        if xab is not None:
            if add_input or fork or C % 4 or C > 256:
                raise TcctError('dwconv3x3(deferred=...): plain convolution with C % 4 == 0, C <= 256 only')
            sums = None
            if stats_box is not None:
                sums = stats_box[1] = _zeros((2 * C,), torch.float64, x.device)
            lib.dwconv3x3_fwd_xaff(x, xab, w, bias, y, N, H, W, C, stride, sums, dtype_code(x.dtype))
        elif stats_box is not None and C % 4 == 0 and C <= 256:
            sums = stats_box[1] = _zeros((2 * C,), torch.float64, x.device)
            lib.dwconv3x3_fwd_bnstats(x, w, bias, y, N, H, W, C, stride, int(add_input), sums, dtype_code(x.dtype))
        else:
            lib.dwconv3x3_fwd(x, w, bias, y, N, H, W, C, stride, int(add_input), dtype_code(x.dtype))
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, add_input, bias is not None)
        ctx.bias_param = bias
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, w = ctx.saved_tensors
        stride, add_input, has_bias = ctx.cfg
        if dy is None:
            return dskip, None, None, None, None, None, None, None, None
        dy = _as(dy, x.dtype)
        N, H, W, C = x.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if dskip is not None:
                lib.dwconv3x3_dgrad_add(dy, w, _as(dskip, x.dtype), dx, N, H, W, C, stride, int(add_input), dtype_code(x.dtype))
            elif ctx.xab is not None and ctx.xlink is not None and stride == 1 and BN_FUSE_RED and BN_RED_DW:
                # x is y_prev of the pending BatchNorm: its two backward sums come out of this launch (raw form), its own reduction pass is skipped
                raw = _zeros((2 * C,), torch.float64, x.device)
                lib.dwconv3x3_dgrad_bnred(dy, w, x, ctx.xab, dx, raw, N, H, W, C, dtype_code(x.dtype))
                ctx.xlink.sums = raw
            else:
                lib.dwconv3x3_dgrad(dy, w, dx, N, H, W, C, stride, int(add_input), dtype_code(x.dtype))
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            # on the weight-gradient side stream like the dense convolutions' (round 4, last day: the ten depthwise weight gradients were 0.85 ms of the
            # ViT branch's input-gradient chain; `DW_WGRAD_SIDE = False` / bench.py --set DW_WGRAD_SIDE=0 keeps them inline)
            keep = (x, dy) if ctx.xab is None else (x, dy, ctx.xab)
            with _wgrad_stream(DW_WGRAD_SIDE and _slot_written(w, ctx.bias_param if has_bias else None), *keep):
                dw = _grad_out(w)
                db = _grad_out(ctx.bias_param) if has_bias else None
                if ctx.xab is not None:
                    lib.dwconv3x3_wgrad_xaff(x, ctx.xab, dy, dw, db, N, H, W, C, stride, dtype_code(x.dtype))
                else:
                    lib.dwconv3x3_wgrad(x, dy, dw, db, N, H, W, C, stride, dtype_code(x.dtype))
        return dx, _ret(dw, w), _ret(db, ctx.bias_param), None, None, None, None, None, None


def dwconv3x3(x, w, bias=None, stride=1, add_input=False, bn_stats=False, deferred=None):
    """bn_stats: a train-mode BatchNorm (no activation in front) consumes the output: its statistics come out of the same launch (`_bn_sums`).
    deferred: the BnLink of a BatchNorm + Hardswish whose normalisation is pending on x (batchnorm_deferred / pw_conv_bn(defer_apply=True))"""
    xab = deferred.ab if deferred is not None else None
    box = _stats_box('none') if bn_stats else None
    return _tag_bn_sums(_DwConv.apply(x, w, bias, stride, add_input, False, box, xab, deferred), box)


def dwconv3x3_fork(x, w, bias=None, stride=1, add_input=False):
    """(dwconv3x3(x), x'): x' aliases x for the other consumers of x (see _DwConv.forward `fork`)"""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return dwconv3x3(x, w, bias, stride, add_input), x
    return _DwConv.apply(x, w, bias, stride, add_input, True)


# ------------------------------------------------------------------------------------------------- norms
def _bn_batch_sums(x, pre, C, M, dc):
    """[sum | sum of squares] (fp64 [2C]) of pre(x) per channel: what the producing convolution's epilogue accumulated (`_bn_sums`, _tag_bn_sums) when it was
    taken behind the same pre-activation at this width, else one tcct_bn_stats launch (which clears its output itself outside a pooled step)"""
    fused = getattr(x, '_bn_sums', None)
    if fused is not None and fused[1] == pre and fused[0].numel() == 2 * C:
        return fused[0]
    sums = ZERO.get((2 * C,), torch.float64, x.device)
    lib.bn_stats(x, M, C, pre, sums, dc)
    return sums


def _bn_coef_bufs(C, device):
    """(mean_rstd, ab): {mean[C], rstd[C]} and {a[C], b[C]} of y = a x + b, written by the launch that finalises the statistics and kept for the backward"""
    return torch.empty(2 * C, device=device, dtype=torch.float32), torch.empty(2 * C, device=device, dtype=torch.float32)


def _bn_backward(ctx, dy):
    """-> (dx, dgamma, dbeta) of a train-mode BatchNorm node that saved (x, gamma, mean_rstd, ab) and set cfg = (pre, post), beta_param, link"""
    x, gamma, mean_rstd, ab = ctx.saved_tensors
    pre, post = ctx.cfg
    dy = _as(dy, x.dtype)
    C = x.shape[-1]
    M = x.numel() // C
    dc = dtype_code(x.dtype)
    link = ctx.link
    if link is not None and link.sums is not None:      # the consumer's input-gradient kernel accumulated the two batch sums (raw form)
        sums = torch.empty(2 * C, device=x.device, dtype=torch.float64)
        lib.bn_sums_from_raw(link.sums, mean_rstd, C, sums)
        link.sums = None
    else:
        sums = ZERO.get((2 * C,), torch.float64, x.device)
        lib.bn_bwd_reduce(x, dy, M, C, mean_rstd, ab, pre, post, sums, dc)
    dx = torch.empty_like(x)
    dg, db = _written_grad_out(gamma, C), _written_grad_out(ctx.beta_param, C)
    lib.bn_bwd_apply(x, dy, dx, M, C, mean_rstd, ab, gamma, sums, pre, post, dg, db, dc)
    return dx, _ret(dg, gamma), _ret(db, ctx.beta_param)


class _BatchNorm(_FastFunction):
    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, eps, momentum, pre, post, training, res=None, link=None):
        _chk(x, gamma, beta)
        C = x.shape[-1]
        M = x.numel() // C
        dc = dtype_code(x.dtype)
        mean_rstd, ab = _bn_coef_bufs(C, x.device)
        if training:
            sums = _bn_batch_sums(x, pre, C, M, dc)
        else:
            lib.bn_eval_ab(C, gamma, beta, eps, rm, rv, mean_rstd, ab)
        y = torch.empty_like(x)
        if res is not None:
            _chk(res)
            if res.shape != x.shape or res.dtype != x.dtype:
                raise TcctError('batchnorm: residual must have the shape and dtype of the input')
        if training:            # statistics finalisation (+ running stats) folded into the apply launch
            lib.bn_apply_train(x, res, y, M, C, sums, gamma, beta, eps, momentum, rm, rv, nbt, mean_rstd, ab, pre, post, dc)
        elif res is not None:
            lib.bn_apply_add(x, res, y, M, C, ab, pre, post, dc)
        else:
            lib.bn_apply(x, y, M, C, ab, pre, post, dc)
        if training:
            ctx.save_for_backward(x, gamma, mean_rstd, ab)
            ctx.cfg = (pre, post)
            ctx.beta_param = beta
            ctx.has_res = res is not None
            ctx.link = link
            if link is not None:
                link.y, link.ab = x, ab
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.has_res:         # the residual receives the gradient as the kernels read it
            dy = _as(dy, ctx.saved_tensors[0].dtype)
        return _bn_backward(ctx, dy) + (None, None, None, None, None, None, None, None, (dy if ctx.has_res else None), None)


# ---- BatchNorm backward folded into the neighbouring pointwise-convolution kernels (round 3) ------------------------------------------
# A train-mode BatchNorm costs 2 (apply) + 2 (backward reduce) + 3 (backward apply) tensor passes.  Where a 1x1 convolution PRODUCES the
# BatchNorm's input (Conv2d_BN, DWConv2d_BN.pwconv, FTC.tran_*), the fused pointwise backward kernel rebuilds the convolution's output
# gradient from (dz, y) while staging its tiles (tcct_pw_bwd_bn): the backward apply pass disappears (3 passes -> 1 extra read).  Where a
# 1x1 convolution CONSUMES a BatchNorm's output as the last contributor to its gradient, the same kernel accumulates that BatchNorm's two
# backward sums in its dx epilogue (`BnLink`): the backward reduce pass disappears too (2 passes -> 1 extra read).  `BN_FUSE = False` (bench.py --set BN_FUSE=0) restores
# the separate kernels (A/B timing, bisecting).
BN_FUSE = True
BN_FUSE_RED = True       # False: keep the separate reduction kernels (A/B timing of the epilogue form)


class BnLink:
    """What a consumer needs to run the backward REDUCTION of the BatchNorm that produced its input: y (the BatchNorm input), ab = {a[C], b[C]},
    the post-activation kind; `sums` is filled (raw form {sum dz', sum dz' y}, fp64 [2C]) by the consumer's backward, which autograd runs
    before the BatchNorm's own backward node -- that node then skips its reduction kernel."""
    __slots__ = ('y', 'ab', 'post', 'sums')

    def __init__(self, y, ab, post):
        self.y, self.ab, self.post, self.sums = y, ab, post, None


def _bn_link_of(x, final):
    """the BnLink of tensor x when x is the unmodified output of a BatchNorm node and the caller vouches (`final`) that its convolution's
    input gradient (+ the forked alias' gradient) is the COMPLETE gradient of x"""
    if not (final and BN_FUSE and BN_FUSE_RED):
        return None
    return getattr(x, '_bn_link', None)


class _PwConvBN(_FastFunction):
    """z = post(BN_train(conv1x1(x))) [+ res] as ONE autograd node (Conv2d_BN / DWConv2d_BN.pwconv / FTC.tran_*, reference nets/tcct.py:55-97,
    124-126,966-974): forward = the GEMM with the statistics in its epilogue + the normalisation pass; backward = [reduction, unless a consumer
    delivered the sums through `link`] + ONE kernel for BatchNorm backward apply, dx, dW, dbias (tcct_pw_bwd_bn), optionally with the reduction
    of the BatchNorm in FRONT of the convolution in its epilogue (`prev`).  x2: second half of a concatenated input (MHCA_stage.aggregate)."""

    @staticmethod
    def forward(ctx, x, x2, w, bias, gamma, beta, rm, rv, nbt, eps, momentum, post, res, fork, link, prev, xdef=None, defer_apply=False):
        """xdef (round 4): x is NOT the convolution's input but y_prev, the input of a train-mode BatchNorm + Hardswish in front whose normalisation
        was deferred (batchnorm_deferred): xdef = its {a[K], b[K]}; the kernels apply hswish(a y_prev + b) while they stage their tiles"""
        ctx.set_materialize_grads(False)
        _chk(x, x2, w, bias, gamma, beta, res)
        K1 = x.shape[-1]
        K = K1 + (x2.shape[-1] if x2 is not None else 0)
        N = w.shape[0]
        M = x.numel() // K1
        y = torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=x.dtype)
        sums = _zeros((2 * N,), torch.float64, x.device)
        if xdef is not None:
            lib.pw_fwd_bnstats_xaff(x, xdef, w, bias, y, M, K, N, sums)
        elif x2 is not None:
            lib.pw_fwd_cat2(x, x2, K1, w, bias, y, M, K, N, sums, 0)
        else:
            lib.pw_fwd_bnstats(x, w, bias, y, M, K, N, sums, 0)
        mean_rstd, ab = _bn_coef_bufs(N, x.device)
        if defer_apply:     # round 4: the normalisation pass is left to the one consumer (a depthwise convolution built with `deferred=link`): z is never written
            lib.bn_finalize(sums, M, N, gamma, beta, eps, momentum, rm, rv, nbt, mean_rstd, ab)
            z = y.view_as(y)
        else:
            z = torch.empty_like(y)
            lib.bn_apply_train(y, res, z, M, N, sums, gamma, beta, eps, momentum, rm, rv, nbt, mean_rstd, ab, 0, post, dtype_code(y.dtype))
        ctx.save_for_backward(x, x2, w, y, mean_rstd, ab)
        wsrc = _param_of(w)
        ctx.cfg = (post, res is not None, wsrc, bias, gamma, beta, link, prev, M, K, N)
        ctx.xdef = xdef
        link.y, link.ab = y, ab
        return (z, x.view_as(x)) if fork else z

    @staticmethod
    def backward(ctx, dz, dalias=None):
        x, x2, w, y, mean_rstd, ab = ctx.saved_tensors
        post, has_res, wsrc, bsrc, gamma, beta, link, prev, M, K, N = ctx.cfg
        if dz is None:
            return (dalias,) + (None,) * 17
        dz = _as(dz, y.dtype)
        if link.sums is not None:               # a consumer's dx epilogue already holds the two batch sums (raw form)
            sums, raw = link.sums, 1
            link.sums = None
        else:
            sums, raw = ZERO.get((2 * N,), torch.float64, y.device), 0
            lib.bn_bwd_reduce(y, dz, M, N, mean_rstd, ab, 0, post, sums, dtype_code(y.dtype))
        dg, db_ = _written_grad_out(gamma, N), _written_grad_out(beta, N)
        dx = torch.empty_like(x)
        dx2 = torch.empty_like(x2) if x2 is not None else None
        dw = _grad_out(wsrc, tuple(w.shape))
        dbias = _grad_out(bsrc) if bsrc is not None else None
        ypv = abp = sp = None
        redp = -1
        if prev is not None:
            redp = prev.post
            ypv, abp = prev.y, prev.ab
            sp = prev.sums = ZERO.get((2 * x.shape[-1],), torch.float64, y.device)
        dskip = _as(dalias, x.dtype) if dalias is not None else None
        if ctx.xdef is not None:        # x is y_prev: the operand is rebuilt on load (dx is the gradient of the DEFERRED BatchNorm's output)
            lib.pw_bwd_bn_sums_xaff(x, ctx.xdef, dz, y, sums, raw, mean_rstd, ab, dg, db_, w, dskip, dx, dw, dbias, M, K, N, redp, sp)
        else:
            lib.pw_bwd_bn_sums(x, x2, dz, y, sums, raw, mean_rstd, ab, dg, db_, post, w, dskip, dx, dx2, dw, dbias, M, K, N, ypv, abp, redp, sp)
        return (dx, dx2, _ret(dw, wsrc), _ret(dbias, bsrc), _ret(dg, gamma), _ret(db_, beta), None, None, None, None, None, None,
                (dz if has_res else None), None, None, None, None, None)


class _Affine2Add(_FastFunction):
    """z = BN1(y1) + BN2(y2) with both normalisations PENDING on their inputs (pw_conv_bn(defer_apply=True) with no activation): one pass; the gradient of z is
    the gradient of both BatchNorm outputs"""

    @staticmethod
    def forward(ctx, y1, ab1, y2, ab2, link1=None, link2=None):
        _chk(y1, ab1, y2, ab2)
        z = torch.empty_like(y1)
        C = y1.shape[-1]
        lib.affine2_add(y1, ab1, y2, ab2, z, y1.numel() // C, C, dtype_code(y1.dtype))
        ctx.links = (link1, link2)
        if link1 is not None and link2 is not None:
            ctx.save_for_backward(y1, y2)
        return z

    @staticmethod
    def backward(ctx, dz):
        l1, l2 = ctx.links
        if l1 is not None and l2 is not None and BN_FUSE_RED and TRAN_RED2:
            # both BatchNorms receive dz: their backward sums (raw form, through the links) from ONE pass over dz, y1, y2
            y1, y2 = ctx.saved_tensors
            dz = _as(dz, y1.dtype)
            C = y1.shape[-1]
            dev = y1.device
            r1 = _zeros((2 * C,), torch.float64, dev)
            r2 = _zeros((2 * C,), torch.float64, dev)
            lib.bn_bwd_reduce2_raw(y1, y2, dz, y1.numel() // C, C, r1, r2, dtype_code(y1.dtype))
            l1.sums, l2.sums = r1, r2
        return dz, None, dz, None, None, None


TRAN_RED2 = True      # False: the two fused BatchNorms keep separate backward reduction passes (A/B timing)
TRAN_FUSE = True      # False: the two BatchNorms of the encoder fusion keep their own normalisation passes (A/B timing)


def affine2_add(y1, link1, y2, link2):
    """BN1(y1) + BN2(y2) for two tensors that carry a pending train-mode BatchNorm (links from pw_conv_bn(..., defer_apply=True))"""
    if y1.shape != y2.shape or y1.dtype != y2.dtype or y1.shape[-1] % 8:
        raise TcctError('affine2_add: two NHWC tensors of one shape and dtype, channels a multiple of 8')
    return _Affine2Add.apply(y1, link1.ab, y2, link2.ab, link1, link2)


BN_RED_DW = True      # False: the BatchNorms in front of the depthwise convolutions keep their backward reduction pass (A/B)
BN_DEFER_DW = True  # False: the BatchNorms in front of the depthwise convolutions keep their normalisation pass (A/B timing)
BN_DEFER = True        # False: InvRes.norm keeps its own normalisation pass (round-3 form; A/B timing)


class _BatchNormDeferred(_FastFunction):
    """A train-mode BatchNorm (+ Hardswish) whose normalisation pass is NOT run (round 4): the node finalises the batch statistics (mean / rstd / a / b,
    running statistics) and returns an ALIAS OF ITS INPUT; the one consumer -- a 1x1 convolution built with `xdef` (pw_conv_bn(..., deferred=link)) --
    applies z = hswish(a y + b) while it stages its tiles.  The gradient that arrives here is the gradient of that virtual z, so the backward is the
    ordinary BatchNorm backward (reduction, unless the consumer's epilogue delivered the sums through `link`, then the apply pass).
    The alias must go to that consumer and nowhere else."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, eps, momentum, post, link):
        _chk(x, gamma, beta)
        C = x.shape[-1]
        M = x.numel() // C
        sums = _bn_batch_sums(x, 0, C, M, dtype_code(x.dtype))
        mean_rstd, ab = _bn_coef_bufs(C, x.device)
        lib.bn_finalize(sums, M, C, gamma, beta, eps, momentum, rm, rv, nbt, mean_rstd, ab)
        ctx.save_for_backward(x, gamma, mean_rstd, ab)
        ctx.cfg = (0, post)
        ctx.beta_param = beta
        ctx.link = link
        link.y, link.ab = x, ab
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        return _bn_backward(ctx, dy) + (None,) * 7


def batchnorm_deferred_ok(x, bn_training, post_act):
    return (BN_DEFER and BN_FUSE and bn_training and torch.is_grad_enabled() and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[-1] in (64, 96)
            and ACT[post_act] == ACT['hswish'] and x.numel() * 2 < 2 ** 31)


def batchnorm_deferred(x, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, post_act):
    """-> (alias of x carrying the pending normalisation, link): hand both to pw_conv_bn(alias, ..., deferred=link) and to nothing else"""
    link = BnLink(None, None, ACT[post_act])
    y = _BatchNormDeferred.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked, float(eps), float(momentum), ACT[post_act], link)
    return y, link


def pw_conv_bn_ok(x, w, bias, bn_training, pre_act, post_act, x2=None, prev=None):
    """shapes / modes the fused node takes: train mode with gradients, bf16 rows, 1x1 weights, K and N in the kernel's table"""
    if not (BN_FUSE and bn_training and torch.is_grad_enabled() and ACT[pre_act] == 0):
        return False
    if x.dtype != torch.bfloat16 or x.dim() != 4 or not x.is_cuda or (w.dim() == 4 and tuple(w.shape[2:]) != (1, 1)):
        return False
    K = x.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
    N = w.shape[0]
    if x2 is not None and not (x.shape[-1] == 64 and x2.shape == x.shape and x2.dtype == x.dtype):
        return False
    M = x.numel() // x.shape[-1]
    if w.shape[1] != K or M * max(K, N) * 2 >= 2 ** 31:
        return False
    return bool(lib.pw_bwd_bn_supported(K, N, ACT[post_act], -1 if prev is None else prev.post, 1 if x2 is not None else 0))


def pw_conv_bn(x, w, bias, bn, post_act=None, residual=None, fork=False, x2=None, x_final=False, deferred=None, defer_apply=False):
    """post_act(BN_train(conv1x1(x [| x2]))) [+ residual]; bn = (gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum).
    fork: also return an alias of x for its other consumers (their gradient is added in this node's dx epilogue).  x_final: this
    convolution's input gradient (+ the alias') is the complete gradient of x -- when x came out of a BatchNorm node, that BatchNorm's
    backward reduction rides on this node's kernel.  Check pw_conv_bn_ok first."""
    gamma, beta, rm, rv, nbt, eps, mom = bn
    link = BnLink(None, None, ACT[post_act])
    w4 = w.view(w.shape[0], w.shape[1], 1, 1) if w.dim() == 2 else w
    if deferred is not None:
        # x is the alias batchnorm_deferred returned: y_prev with z = hswish(a y_prev + b) pending; K = N = 64 also carries that BatchNorm's
        # backward reduction in its dx epilogue (the kernel table of tcct_pw_bwd_bn_sums_xaff), 96 leaves it to the BatchNorm's own node
        if post_act is not None or fork or x2 is not None or x.shape[-1] != w.shape[0] or x.shape[-1] not in (64, 96):
            raise TcctError('pw_conv_bn(deferred=...): square 64 / 96 convolution without activation, fork or concatenation only')
        prev = deferred if (x.shape[-1] == 64 and BN_FUSE_RED) else None
        out = _PwConvBN.apply(x, None, w4, bias, gamma, beta, rm, rv, nbt, float(eps), float(mom), 0, residual, False, link, prev, deferred.ab)
        out._bn_link = link
        return out
    prev = _bn_link_of(x, x_final)
    if prev is not None and not pw_conv_bn_ok(x, w, bias, True, None, post_act, x2, prev):
        prev = None
    if defer_apply:
        # the caller hands the result (y with the normalisation + Hardswish PENDING) and `link` to dwconv3x3(..., deferred=link) and to nothing else
        if residual is not None or x2 is not None or ACT[post_act] not in (ACT['hswish'], ACT['none']):
            raise TcctError('pw_conv_bn(defer_apply=True): BatchNorm (+ Hardswish) without residual / concatenation only')
        out = _PwConvBN.apply(x, None, w4, bias, gamma, beta, rm, rv, nbt, float(eps), float(mom), ACT[post_act], None, fork, link, prev, None, True)
        return out, link
    out = _PwConvBN.apply(x, x2, w4, bias, gamma, beta, rm, rv, nbt, float(eps), float(mom), ACT[post_act], residual, fork, link, prev)
    z = out[0] if fork else out
    z._bn_link = link               # (with a residual folded in z is BN output + res, but the gradient of the BatchNorm output still is dz)
    return out


BN_POOL_FUSE = True      # False: BatchNorm pass, then the pooling pass (A/B timing)


class LazyGrad:
    """A gradient that travels beside autograd as a RECIPE, and the only place that knows what its placeholder is.  One link per forward node of a PRODUCER
    whose backward kernels can form the gradient of its output t on load (_NormAdd / _NormAdd6: `feats`; _BnPoolFork: the level-0 skip z); the producer's ctx
    owns it.  A CONSUMER whose d loss / dt is cheap to describe (_Fpl: a (labels, bins, table) lookup; the composed level-0 head: Wb^T dl, rank n_class) calls
    `file` in its backward and returns the placeholder -- a zero-stride expansion of one zero element: right shape and dtype, no memory -- to autograd.  The
    producer's backward calls `take(dy)`: the single untouched placeholder means its fused kernels run on the recipe; a placeholder that autograd ADDED to
    another consumer's gradient (or to another placeholder) arrives as a dense tensor that lacks the filed parts, and every recipe has to be materialised and
    added (_add_materialised).  ok: the producer has the fused kernels for its shape / kinds.

    How a consumer finds the link: the skip edge carries it as a tensor attribute (`z._skip0`, forwarded by grad_mark); `feats` reaches RegNet.regular_udh as
    an NCHW view of a view through the reference's public `base.feats` protocol, which attributes do not survive, so _NormAdd / _NormAdd6 `register` their
    output's address for the step and _Fpl looks it up (`of`); begin_step resets the registry, and an entry is void once the producer's node is gone.
    HAZARD: the registry cannot tell a registered tensor from a later one that the allocator put at the same address while the producer's node is still
    alive (its output freed, an alias of its inputs still held) -- a recipe filed on such a tensor would reach that producer's link and be lost to the
    tensor's real one.  Nothing here detects it; FTC keeps `feats` alive until the next forward pass (`_feats`), so a training step does not meet it.
    LIMITATION (only what exists when the consumer's forward runs is visible to grad_is_watched): `torch.autograd.grad(loss, t)` and a hook registered on t
    AFTER the consumer ran receive the all-zero placeholder; the real gradient still reaches every weight.  A caller who wants to SEE the dense d loss / dt
    calls `t.retain_grad()` / registers the hook BEFORE the consumer runs (RegNet.regular_udh, the head), or `ops.fpl(..., allow_lazy=False)`, or clears
    `ops.FPL_LAZY_GRAD` / `ops.SKIP0_LOWRANK`."""
    __slots__ = ('ok', 'recipes', '__weakref__')
    _by_address = {}        # data_ptr of a registered producer output -> weak reference to its link, for the running step

    def __init__(self, ok=True):
        self.ok, self.recipes = bool(ok), []

    def register(self, t):
        LazyGrad._by_address[t.data_ptr()] = weakref.ref(self)      # weak: the producer's ctx owns the link, an entry dies with the producer's node

    @staticmethod
    def of(t):
        ref = LazyGrad._by_address.get(t.data_ptr())
        return ref() if ref is not None else None

    def file(self, recipe, shape, dtype, device):
        """consumer side: keep (marker, *recipe) for the producer, -> the placeholder to return to autograd as the gradient"""
        marker = torch.zeros(1, device=device, dtype=dtype)
        self.recipes.append((marker,) + tuple(recipe))
        return marker.expand(shape)

    def take(self, dy):
        """producer side, dy = what autograd delivered (or None) -> (single, rest) and the link is empty again.  single: the one filed recipe when dy is
        exactly its untouched placeholder (the caller forms the gradient from it; dy holds nothing); otherwise None, and rest lists the recipes to materialise
        and add to the dense dy.  Tensor metadata only: no kernel, no library call."""
        recipes, self.recipes = self.recipes, []
        if len(recipes) == 1 and dy is not None and dy.dim() == 4 and dy.stride(0) == 0 and dy.data_ptr() == recipes[0][0].data_ptr():
            return recipes[0], []
        return None, recipes


def fpl_lazy_grad_reset():
    """per step (begin_step): forget last step's registered producer outputs (storage addresses are recycled by the allocator)"""
    LazyGrad._by_address.clear()


def lazy_grads_pending(*links):
    """number of recipes filed and not yet taken, on the registered links and on `links` (0 after a complete backward pass)"""
    live = {ref() for ref in LazyGrad._by_address.values()} - {None}
    return sum(len(k.recipes) for k in live | set(links))


def _add_materialised(dy, recipes, like, materialise):
    """dy (dense, or None) + every recipe as a tensor like `like`: materialise(recipe, out) launches the consumer's dense gradient kernel, then the sum"""
    dy = None if dy is None else _as(dy, like.dtype)
    for recipe in recipes:
        d = torch.empty_like(like)
        materialise(recipe, d)
        dy = d if dy is None else add(dy, d)
    return dy


def bn_pool_lowrank_ok(x, pre, post):
    """tcct_bn_pool_bwd_lowrank's own test: bf16, 32 channels, LeakyReLU in front and nothing behind (the CNN encoder's level 0)"""
    return x.dtype == torch.bfloat16 and x.shape[-1] == 32 and pre == ACT['lrelu'] and post == ACT['none']


class _BnPoolFork(_FastFunction):
    """(maxpool2(z), z) with z = post(BN_train(pre(x))) from ONE pass over x (tcct_bn_pool_fwd_train); in the backward pass the gradient of
    z -- the skip consumers' gradient plus the pooling scatter -- is never written: both BatchNorm backward kernels rebuild it from its
    two sources (tcct_bn_pool_bwd).  Encoder levels 0-3 (reference nets/tcct.py:820-823, :876-884)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, eps, momentum, pre, post, link=None):
        ctx.set_materialize_grads(False)
        _chk(x, gamma, beta)
        N, H, W, C = x.shape
        dc = dtype_code(x.dtype)
        ctx.link = link
        sums = _bn_batch_sums(x, pre, C, N * H * W, dc)
        mean_rstd, ab = _bn_coef_bufs(C, x.device)
        z = torch.empty_like(x)
        pooled = torch.empty((N, H // 2, W // 2, C), device=x.device, dtype=x.dtype)
        amax = torch.empty((N, H // 2, W // 2, C // 4), device=x.device, dtype=torch.uint8)        # 2-bit window positions of the maxima
        lib.bn_pool_fwd_train(x, z, pooled, amax, N, H, W, C, sums, gamma, beta, eps, momentum, rm, rv, nbt, mean_rstd, ab, pre, post, dc)
        ctx.save_for_backward(x, mean_rstd, ab, amax)
        ctx.cfg = (pre, post, gamma, beta)
        return pooled, z

    @staticmethod
    def backward(ctx, dpool, dskip):
        x, mean_rstd, ab, amax = ctx.saved_tensors
        pre, post, gamma, beta = ctx.cfg
        N, H, W, C = x.shape
        dc = dtype_code(x.dtype)
        if dpool is None and dskip is None:
            return (None,) * 11
        # (dl, wb, n_class) recipes the composed head filed instead of a dense gradient of z (SKIP0_LOWRANK)
        lowrank, rest = ctx.link.take(dskip) if ctx.link is not None else (None, [])
        if lowrank is not None:
            dskip = None
        elif rest:
            dskip = _add_materialised(dskip, rest, x, lambda r, d: lib.conv2d_dgrad(r[1], r[2], d, N, H, W, C, r[3], 1, 1, 0, 0, dtype_code(torch.float32), dc))
        if dpool is None:           # only the full-size output was used: a plain BatchNorm backward
            dpool = torch.zeros((N, H // 2, W // 2, C), device=x.device, dtype=x.dtype)      # an INPUT of the kernel: must really be zero
        dpool = _as(dpool, x.dtype)
        if dskip is not None:
            dskip = _as(dskip, x.dtype)
        sums = ZERO.get((2 * C,), torch.float64, x.device)
        dx = torch.empty_like(x)
        dg, db = _written_grad_out(gamma, C), _written_grad_out(beta, C)
        if lowrank is not None:
            _, dl, wb, nc = lowrank
            keep_until_end_of_step(dl, wb, torch.cuda.current_stream())     # handed over beside autograd: nothing else ties their lifetime to this stream
            lib.bn_pool_bwd_lowrank(x, dpool, dl, wb, nc, amax, dx, N, H, W, C, mean_rstd, ab, pre, post, sums, dg, db, dc)
        else:
            lib.bn_pool_bwd(x, dpool, dskip, amax, dx, N, H, W, C, mean_rstd, ab, pre, post, sums, dg, db, dc)
        return dx, _ret(dg, gamma), _ret(db, beta), None, None, None, None, None, None, None, None


def bn_pool_ok(x, training):
    """shapes the fused BatchNorm + MaxPool2d(2) kernels take (train mode, gradients wanted): even extents, C/4 dividing 256"""
    N, H, W, C = x.shape
    return (BN_POOL_FUSE and training and torch.is_grad_enabled() and x.requires_grad and C % 4 == 0 and C <= 256 and 256 % (C // 4) == 0
            and H % 2 == 0 and W % 2 == 0 and H >= 2 and W >= 2)


def batchnorm_maxpool2_fork(x, gamma, beta, running_mean, running_var, num_batches_tracked=None, eps=1e-5, momentum=0.1, pre_act=None,
                            post_act=None):
    """(maxpool2(z), z), z = post_act(BN_train(pre_act(x))): see _BnPoolFork; check bn_pool_ok(x, training) first"""
    link = LazyGrad(bn_pool_lowrank_ok(x, ACT[pre_act], ACT[post_act]))
    pooled, z = _BnPoolFork.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked, float(eps), float(momentum), ACT[pre_act], ACT[post_act], link)
    z._skip0 = link         # what the composed level-0 head (_UpSkipConvT32AuxLow) looks for on its skip input
    return pooled, z


def batchnorm(x, gamma, beta, running_mean, running_var, num_batches_tracked=None, eps=1e-5, momentum=0.1,
              pre_act=None, post_act=None, training=True, residual=None):
    """y = post_act(BN(pre_act(x))) [+ residual] over the last (channel) dim, torch train-mode semantics incl. running stats."""
    if not training and torch.is_grad_enabled() and x.requires_grad:
        raise TcctError('eval-mode batchnorm is inference-only here')
    link = None
    if (BN_FUSE and training and torch.is_grad_enabled() and x.dtype == torch.bfloat16 and ACT[pre_act] == 0
            and ACT[post_act] in (0, 2) and x.shape[-1] in (64, 96, 128)):
        link = BnLink(None, None, ACT[post_act])       # a pointwise convolution that consumes the output may run this node's backward reduction
    z = _BatchNorm.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked, float(eps), float(momentum),
                         ACT[pre_act], ACT[post_act], bool(training), residual, link)
    if link is not None:
        z._bn_link = link
    return z


class _Bn2AddAct(_FastFunction):
    """y = act(BN_A(pre(xa)) + BN_B(pre(xb))), both BatchNorms in train mode (CrossCNNBlock junction)"""

    @staticmethod
    def forward(ctx, xa, gA, bA, xb, gB, bB, bufs, eps, momentum, pre, act_kind):
        _chk(xa, xb, gA, bA, gB, bB)
        C = xa.shape[-1]
        M = xa.numel() // C
        dc = dtype_code(xa.dtype)
        st, ss = [], []
        for x in (xa, xb):
            st += _bn_coef_bufs(C, x.device)
            ss.append(_bn_batch_sums(x, pre, C, M, dc))
        y = torch.empty_like(xa)
        (rmA, rvA, nbtA), (rmB, rvB, nbtB) = bufs       # both statistics finalisations ride on the junction launch
        lib.bn2_add_act_train(xa, xb, y, M, C, ss[0], gA, bA, rmA, rvA, nbtA, st[0], st[1], ss[1], gB, bB, rmB, rvB, nbtB, st[2], st[3],
                              eps, momentum, pre, act_kind, dc)
        ctx.save_for_backward(xa, xb, *st)
        ctx.cfg = (pre, act_kind)
        ctx.params = (gA, bA, gB, bB)
        return y

    @staticmethod
    def backward(ctx, dy):
        xa, xb, mrA, abA, mrB, abB = ctx.saved_tensors
        pre, act_kind = ctx.cfg
        gA, bA, gB, bB = ctx.params
        dy = _as(dy, xa.dtype)
        C = xa.shape[-1]
        M = xa.numel() // C
        dc = dtype_code(xa.dtype)
        sums = ZERO.get((4 * C,), torch.float64, xa.device)
        lib.bn2_add_act_bwd_reduce(xa, xb, dy, M, C, mrA, abA, mrB, abB, pre, act_kind, sums, dc)
        dxa, dxb = torch.empty_like(xa), torch.empty_like(xb)
        outs = [_written_grad_out(p, C) for p in (gA, bA, gB, bB)]
        lib.bn2_add_act_bwd_apply(xa, xb, dy, dxa, dxb, M, C, mrA, abA, mrB, abB, sums, pre, act_kind, outs[0], outs[1], outs[2],
                                  outs[3], dc)
        return (dxa, _ret(outs[0], gA), _ret(outs[1], bA), dxb, _ret(outs[2], gB), _ret(outs[3], bB), None, None, None, None, None)


def bn2_add_act(xa, bnA, xb, bnB, pre_act='lrelu', act_kind='gelu'):
    """bnA/bnB: (gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum) of the two train-mode BatchNorms"""
    gA, bA, rmA, rvA, nbtA, eps, mom = bnA
    gB, bB, rmB, rvB, nbtB, _, _ = bnB
    return _Bn2AddAct.apply(xa, gA, bA, xb, gB, bB, ((rmA, rvA, nbtA), (rmB, rvB, nbtB)), float(eps), float(mom), ACT[pre_act],
                            ACT[act_kind])


def _layernorm_backward(x, dy, dskip, gamma, beta, mr):
    """-> (dx, dgamma, dbeta) of y = LayerNorm(x) with statistics mr; dskip (or None): a gradient that reaches x around the normalisation, added inside the
    kernel (tcct_layernorm_bwd_add)"""
    C = x.shape[-1]
    M = x.numel() // C
    dx = torch.empty_like(x)
    dg, db = _grad_out(gamma), _grad_out(beta)
    if dskip is None:
        lib.layernorm_bwd(x, dy, dx, M, C, gamma, mr, dg, db, dtype_code(x.dtype))
    else:
        lib.layernorm_bwd_add(x, dy, _as(dskip, x.dtype), dx, M, C, gamma, mr, dg, db, dtype_code(x.dtype))
    return dx, dg, db


class _LayerNorm(_FastFunction):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, fork=False):
        """fork: also return an alias of x for the residual path around the normalisation; its gradient is then added inside the
        LayerNorm backward kernel (tcct_layernorm_bwd_add) instead of by an autograd accumulation pass"""
        ctx.set_materialize_grads(False)      # an unused output must arrive as None in backward(), not as a zero-filled tensor
        _chk(x, gamma, beta)
        C = x.shape[-1]
        M = x.numel() // C
        y = torch.empty_like(x)
        mr = torch.empty(2 * M, device=x.device, dtype=torch.float32)
        lib.layernorm_fwd(x, y, M, C, gamma, beta, eps, mr, dtype_code(x.dtype))
        ctx.save_for_backward(x, gamma, mr)
        ctx.beta_param = beta
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, gamma, mr = ctx.saved_tensors
        if dy is None:
            return dskip, None, None, None, None
        dx, dg, db = _layernorm_backward(x, _as(dy, x.dtype), dskip, gamma, ctx.beta_param, mr)
        return dx, _ret(dg, gamma), _ret(db, ctx.beta_param), None, None


def layernorm(x, gamma, beta, eps=1e-6):
    return _LayerNorm.apply(x, gamma, beta, float(eps), False)


def layernorm_fork(x, gamma, beta, eps=1e-6):
    """(LayerNorm(x), x'): x' aliases x and is to be read by the residual path (see _LayerNorm.forward `fork`)"""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return layernorm(x, gamma, beta, eps), x
    return _LayerNorm.apply(x, gamma, beta, float(eps), True)


# ------------------------------------------------------------------------------------------- elementwise
class _Act(_FastFunction):
    @staticmethod
    def forward(ctx, x, kind):
        _chk(x)
        y = torch.empty_like(x)
        lib.act_fwd(x, y, x.numel(), kind, dtype_code(x.dtype))
        ctx.save_for_backward(x)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _as(dy, x.dtype)
        dx = torch.empty_like(x)
        lib.act_bwd(x, dy, dx, x.numel(), ctx.kind, dtype_code(x.dtype))
        return dx, None


def act(x, kind):
    return _Act.apply(x, ACT[kind])


class _AddAct(_FastFunction):
    @staticmethod
    def forward(ctx, a, b, kind):
        _chk(a, b)
        y = torch.empty_like(a)
        if kind == 0:
            lib.add(a, b, y, a.numel(), dtype_code(a.dtype))
        else:
            lib.add_act_fwd(a, b, y, a.numel(), kind, dtype_code(a.dtype))
            ctx.save_for_backward(a, b)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.kind == 0:
            return dy, dy, None
        a, b = ctx.saved_tensors
        dy = _as(dy, a.dtype)
        dx = torch.empty_like(a)
        lib.add_act_bwd(a, b, dy, dx, a.numel(), ctx.kind, dtype_code(a.dtype))
        return dx, dx, None


def add_act(a, b, kind=None):
    """act(a + b)"""
    return _AddAct.apply(a, b, ACT[kind])


def add(a, b):
    return _AddAct.apply(a, b, 0)


class _Residual(_FastFunction):
    @staticmethod
    def forward(ctx, x, z, scale):
        _chk(x, z, scale)
        B = x.shape[0]
        y = torch.empty_like(x)
        lib.residual_fwd(x, z, scale, y, B, x.numel() // B, dtype_code(x.dtype))
        ctx.save_for_backward(scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        (scale,) = ctx.saved_tensors
        dy = _c(dy)
        return dy, _scale_rows(dy, scale), None


def residual(x, z, scale=None):
    """x + scale[b] * z  (scale: fp32 [B] DropPath mask/keep_prob, or None for a plain add)"""
    if scale is None:
        return add(x, z)
    return _Residual.apply(x, z, scale)


class _Concat2(_FastFunction):
    @staticmethod
    def forward(ctx, a, b):
        _chk(a, b)
        Ca, Cb = a.shape[-1], b.shape[-1]
        M = a.numel() // Ca
        y = torch.empty(a.shape[:-1] + (Ca + Cb,), device=a.device, dtype=a.dtype)
        lib.concat2(a, b, y, M, Ca, Cb, dtype_code(a.dtype))
        ctx.cfg = (Ca, Cb)
        return y

    @staticmethod
    def backward(ctx, dy):
        Ca, Cb = ctx.cfg
        dy = _c(dy)
        M = dy.numel() // (Ca + Cb)
        da = torch.empty(dy.shape[:-1] + (Ca,), device=dy.device, dtype=dy.dtype)
        db = torch.empty(dy.shape[:-1] + (Cb,), device=dy.device, dtype=dy.dtype)
        lib.split2(dy, da, db, M, Ca, Cb, dtype_code(dy.dtype))
        return da, db


def concat2(a, b):
    return _Concat2.apply(a, b)


class _Add3Scale(_FastFunction):
    @staticmethod
    def forward(ctx, a, b, c, alpha):
        _chk(a, b, c)
        y = torch.empty_like(a)
        lib.add3_scale(a, b, c, y, a.numel(), alpha, dtype_code(a.dtype))
        ctx.alpha = alpha
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        d = torch.empty_like(dy)
        lib.scale(dy, d, dy.numel(), ctx.alpha, dtype_code(dy.dtype))
        return d, d, d, None


class _GateFusion(_FastFunction):
    @staticmethod
    def forward(ctx, x1, x2, field):
        _chk(x1, x2, field)
        N, H, W, C = x1.shape
        hs, ws = field.shape[1], field.shape[2]
        if field.dtype != torch.float32 or tuple(field.shape) != (N, hs, ws, C) or x2.shape != x1.shape:
            raise TcctError('gate_fusion: field must be fp32 NHWC [N,hs,ws,C] and x2 like x1')
        y = torch.empty_like(x1)
        lib.gate_fusion_fwd(x1, x2, field, y, N, H, W, C, hs, ws, dtype_code(x1.dtype))
        ctx.save_for_backward(field)
        return y

    @staticmethod
    def backward(ctx, dy):
        (field,) = ctx.saved_tensors
        dy = _c(dy)
        N, H, W, C = dy.shape
        d1, d2 = torch.empty_like(dy), torch.empty_like(dy)
        lib.gate_fusion_bwd(dy, field, d1, d2, N, H, W, C, field.shape[1], field.shape[2], dtype_code(dy.dtype))
        return d1, d2, None


def gate_fusion(x1, x2, field):
    """GateFusion training branch: x1*alpha + x2*(1-alpha), alpha = clamp(bicubic(field -> H x W), 0, 1); field fp32 NHWC [N,hs,ws,C]"""
    return _GateFusion.apply(x1, x2, field)


def add3_scale(a, b, c, alpha):
    return _Add3Scale.apply(a, b, c, float(alpha))


# -------------------------------------------------------------------------------------- pooling / resize
class _MetaPool(_FastFunction):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        B, N, C = x.shape
        y = torch.empty_like(x)
        lib.metapool_fwd(x, y, B, N, C, dtype_code(x.dtype))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        B, N, C = dy.shape
        dx = torch.empty_like(dy)
        lib.metapool_bwd(dy, dx, B, N, C, dtype_code(dy.dtype))
        return dx


class _MetaPoolResidual(_FastFunction):
    """t + scale[b] * metapool(cur): mixer branch, DropPath scale and residual add in one pass (and one pass backward)"""

    @staticmethod
    def forward(ctx, cur, t, scale):
        _chk(cur, t, scale)
        B, N, C = cur.shape
        y = torch.empty_like(cur)
        lib.metapool_residual_fwd(cur, t, scale, y, B, N, C, dtype_code(cur.dtype))
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        B, N, C = dy.shape
        dcur = torch.empty_like(dy)
        lib.metapool_scaled_bwd(dy, ctx.scale, dcur, B, N, C, dtype_code(dy.dtype))
        return dcur, dy, None


def metapool_residual(cur, t, scale=None):
    """t + scale[b] * MetaPool(cur) on tokens [B,N,C] (scale: fp32 [B] or None)"""
    return _MetaPoolResidual.apply(cur, t, scale)


class _LnMetaPoolResidual(_FastFunction):
    """t + scale[b] * (pool(LN(t)) - LN(t)): MHCABlock's first half (reference nets/tcct.py:457-465, MetaPool :405-415) as ONE pass each way
    (csrc/ln_pool.hip): the normalised tensor and its gradient are never written"""

    @staticmethod
    def forward(ctx, t, gamma, beta, eps, scale):
        _chk(t, gamma, beta, scale)
        B, N, C = t.shape
        y = torch.empty_like(t)
        lib.ln_metapool_residual_fwd(t, y, B, N, C, gamma, beta, eps, scale, dtype_code(t.dtype))
        ctx.save_for_backward(t, gamma)
        ctx.beta_param, ctx.scale, ctx.eps = beta, scale, eps
        return y

    @staticmethod
    def backward(ctx, dy):
        t, gamma = ctx.saved_tensors
        dy = _as(dy, t.dtype)
        B, N, C = t.shape
        dt = torch.empty_like(t)
        dg, db = _grad_out(gamma), _grad_out(ctx.beta_param)
        lib.ln_metapool_residual_bwd(t, dy, dt, B, N, C, gamma, ctx.eps, ctx.scale, dg, db, dtype_code(t.dtype))
        return dt, _ret(dg, gamma), _ret(db, ctx.beta_param), None, None


class _LnMetaPoolResidualLn(_FastFunction):
    """(t1, LN2(t1)) with t1 = t + scale[b] * (pool(LN1(t)) - LN1(t)): MHCABlock up to the input of its Mlp (reference nets/tcct.py:457-466) from ONE forward
    pass -- the second LayerNorm is taken of the row while it is in registers.  Backward: LayerNorm-2 backward (+ the residual path's gradient of t1), then
    the one-pass backward of the first half."""

    @staticmethod
    def forward(ctx, t, g1, b1, eps1, scale, g2, b2, eps2):
        ctx.set_materialize_grads(False)
        _chk(t, g1, b1, scale, g2, b2)
        B, N, C = t.shape
        y, y2 = torch.empty_like(t), torch.empty_like(t)
        mr2 = torch.empty(2 * B * N, device=t.device, dtype=torch.float32)
        lib.ln_metapool_residual_ln_fwd(t, y, y2, B, N, C, g1, b1, eps1, scale, g2, b2, eps2, mr2, dtype_code(t.dtype))
        ctx.save_for_backward(t, y, g1, g2, mr2)
        ctx.beta = (b1, b2)
        ctx.cfg = (eps1, scale)
        ctx.mark_non_differentiable(mr2)
        return y, y2, mr2

    @staticmethod
    def backward(ctx, dres, dcur, _dmr=None):
        t, y, g1, g2, mr2 = ctx.saved_tensors
        b1, b2 = ctx.beta
        eps1, scale = ctx.cfg
        B, N, C = t.shape
        dg2 = db2 = None
        if dcur is not None:
            dt1, dg2, db2 = _layernorm_backward(y, _as(dcur, t.dtype), dres, g2, b2, mr2)
        else:
            dt1 = _as(dres, t.dtype)
        dt = torch.empty_like(t)
        dg1, db1 = _grad_out(g1), _grad_out(b1)
        lib.ln_metapool_residual_bwd(t, dt1, dt, B, N, C, g1, eps1, scale, dg1, db1, dtype_code(t.dtype))
        return dt, _ret(dg1, g1), _ret(db1, b1), None, None, _ret(dg2, g2), _ret(db2, b2), None


LN_POOL_FUSE = True       # False: LayerNorm and the token mixer stay separate kernels (A/B timing)


def ln_metapool_residual_ok(t, gamma, beta):
    return (LN_POOL_FUSE and t.dim() == 3 and t.is_cuda and t.is_contiguous() and t.dtype in (torch.float32, torch.bfloat16) and t.shape[-1] % 8 == 0
            and 16 <= t.shape[-1] <= 192 and t.shape[0] <= 65535 and t.shape[1] < 2 ** 30 and gamma is not None and beta is not None)


def ln_metapool_residual(t, gamma, beta, eps=1e-6, scale=None):
    """t + scale[b] * MetaPool(LayerNorm(t)) on tokens [B,N,C] in one pass (scale: fp32 [B] or None); check ln_metapool_residual_ok first"""
    return _LnMetaPoolResidual.apply(t, gamma, beta, float(eps), scale)


LN_POOL_LN2 = True       # False: the second LayerNorm stays its own forward pass (A/B timing)


def ln_metapool_residual_ln(t, g1, b1, eps1, scale, g2, b2, eps2):
    """(t1, LayerNorm2(t1), its statistics [B*N*2]), t1 = t + scale[b] * MetaPool(LayerNorm1(t)): one forward pass; check ln_metapool_residual_ok first"""
    return _LnMetaPoolResidualLn.apply(t, g1, b1, float(eps1), scale, g2, b2, float(eps2))


def metapool(x):
    """x tokens [B,N,C]"""
    return _MetaPool.apply(x)


def _att_check(name, qkv, H, W, heads, wb):
    """the shapes both attention nodes need: qkv [B, H*W, 3C], C a multiple of heads, Ch = C / heads a multiple of 4, the crpe windows covering C"""
    B, N, C3 = qkv.shape
    C = C3 // 3
    if C * 3 != C3 or H * W != N or C % heads or (C // heads) % 4:
        raise TcctError(f'{name}: qkv {tuple(qkv.shape)} does not fit size ({H},{W}) / heads {heads} (Ch must be a multiple of 4)')
    if sum(w.shape[0] for w in wb[0::2]) != C:
        raise TcctError(f'{name}: the crpe window splits do not add up to the channel count')


def _crpe_forward(qkv, H, W, wb):
    """cv [B,N,C] = the depthwise K x K windows of ConvRelPosEnc over the channel groups of v, read in place out of qkv (wb: weight, bias per window)"""
    B, N, C3 = qkv.shape
    C, dt = C3 // 3, dtype_code(qkv.dtype)
    cv = torch.empty((B, N, C), device=qkv.device, dtype=qkv.dtype)
    off = 0
    for w, b in zip(wb[0::2], wb[1::2]):
        Cg, K = w.shape[0], w.shape[2]
        lib.dwk_strided_fwd(qkv[0, 0, 2 * C + off:], 3 * C, w, b, cv[0, 0, off:], C, B, H, W, Cg, K, 0, 0, dt)
        off += Cg
    return cv


def _crpe_backward(qkv, dcv, dqkv, H, W, wb):
    """the windows' backward: the gradient through cv is ADDED to the v third of dqkv; -> what backward returns for wb"""
    B, N, C3 = qkv.shape
    C, dt = C3 // 3, dtype_code(qkv.dtype)
    grads, off = [], 0
    for w, b in zip(wb[0::2], wb[1::2]):
        Cg, K = w.shape[0], w.shape[2]
        lib.dwk_strided_fwd(dcv[0, 0, off:], C, w, None, dqkv[0, 0, 2 * C + off:], 3 * C, B, H, W, Cg, K, 1, 1, dt)
        dw = _grad_out(w)
        db = _grad_out(b) if b is not None else None
        lib.dwk_strided_wgrad(qkv[0, 0, 2 * C + off:], 3 * C, dcv[0, 0, off:], C, dw, db, B, H, W, Cg, K, dt)
        grads += [_ret(dw, w), _ret(db, b)]
        off += Cg
    return tuple(grads)


def _crpe_wb(crpe_convs):
    """the nn.Conv2d list of ConvRelPosEnc -> [weight, bias, weight, bias, ...]"""
    return [p for m in crpe_convs for p in (m.weight, m.bias)]


class _FactorAtt(_FastFunction):
    """FactorAtt_ConvRelPosEnc.forward between the qkv and proj Linear layers (reference nets/tcct.py:316-331 + ConvRelPosEnc.forward
    :265-287): out [B,N,C] = scale * q (softmax_N(k)^T v) + q * crpe(v), qkv [B,N,3C] (dormant in stc_tt)."""

    @staticmethod
    def forward(ctx, qkv, H, W, heads, scale, *wb):
        _chk(qkv, *wb)
        _att_check('factor_att', qkv, H, W, heads, wb)
        B, N, C3 = qkv.shape
        C = C3 // 3
        Ch, dt, dev = C // heads, dtype_code(qkv.dtype), qkv.device
        ws = torch.empty(lib.fatt_kstats_workspace_bytes(B, N, C), device=dev, dtype=torch.uint8)
        stats = torch.empty((B, C, 2), device=dev, dtype=torch.float32)
        lib.fatt_kstats(qkv, ws, stats, B, N, C, heads, dt)
        M = ZERO.get((B, heads, Ch, Ch), torch.float32, dev)
        lib.fatt_ktv(qkv, stats, M, B, N, C, heads, dt)
        cv = _crpe_forward(qkv, H, W, wb)
        out = torch.empty((B, N, C), device=dev, dtype=qkv.dtype)
        lib.fatt_apply_fwd(qkv, M, cv, out, float(scale), B, N, C, heads, dt)
        ctx.save_for_backward(qkv, stats, M, cv, *wb[0::2])
        ctx.cfg = (H, W, heads, float(scale))
        ctx.params = wb
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, stats, M, cv, *ws = ctx.saved_tensors
        H, W, heads, scale = ctx.cfg
        B, N, C3 = qkv.shape
        C = C3 // 3
        dt, dev = dtype_code(qkv.dtype), qkv.device
        dout = _as(dout, qkv.dtype)
        dM = ZERO.get(tuple(M.shape), torch.float32, dev)
        lib.fatt_dktv(qkv, dout, dM, scale, B, N, C, heads, dt)
        dqkv = torch.empty_like(qkv)
        dcv = torch.empty_like(cv)
        lib.fatt_apply_bwd(qkv, stats, M, dM, cv, dout, dqkv, dcv, scale, B, N, C, heads, dt)
        return (dqkv, None, None, None, None) + _crpe_backward(qkv, dcv, dqkv, H, W, ctx.params)


def factor_att(qkv, size, heads, scale, crpe_convs):
    """qkv [B,N,3C] tokens, size = (H, W), crpe_convs = the nn.Conv2d list of ConvRelPosEnc (windows 3/5/7 over head splits)"""
    return _FactorAtt.apply(qkv, int(size[0]), int(size[1]), int(heads), float(scale), *_crpe_wb(crpe_convs))


class _HydraAtt(_FastFunction):
    """HydraAttention.forward between the qkv and proj Linear layers (reference nets/tcct.py:369-397 + ConvRelPosEnc.forward :265-287):
    out [B,N,C] = scale * (q / |q|) * sum_N((k / |k|) * v) + q * crpe(v), qkv [B,N,3C]; norms over the Ch channels of a head, no epsilon."""

    @staticmethod
    def forward(ctx, qkv, H, W, heads, scale, *wb):
        _chk(qkv, *wb)
        _att_check('hydra_att', qkv, H, W, heads, wb)
        B, N, C3 = qkv.shape
        C = C3 // 3
        dt, dev = dtype_code(qkv.dtype), qkv.device
        ws = torch.empty(lib.hydra_kv_workspace_bytes(B, N, C), device=dev, dtype=torch.uint8)
        kv = torch.empty((B, C), device=dev, dtype=torch.float32)
        lib.hydra_kv(qkv, ws, kv, B, N, C, heads, dt)
        cv = _crpe_forward(qkv, H, W, wb)
        out = torch.empty((B, N, C), device=dev, dtype=qkv.dtype)
        lib.hydra_apply_fwd(qkv, kv, cv, out, float(scale), B, N, C, heads, dt)
        # (under no_grad autograd records no node: the context and what it holds are dropped when apply() returns)
        ctx.save_for_backward(qkv, kv, cv, *wb[0::2])
        ctx.cfg = (H, W, heads, float(scale))
        ctx.params = wb
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, kv, cv, *ws = ctx.saved_tensors
        H, W, heads, scale = ctx.cfg
        B, N, C3 = qkv.shape
        C = C3 // 3
        dt, dev = dtype_code(qkv.dtype), qkv.device
        dout = _as(dout, qkv.dtype)
        wsp = torch.empty(lib.hydra_kv_workspace_bytes(B, N, C), device=dev, dtype=torch.uint8)
        dkv = torch.empty((B, C), device=dev, dtype=torch.float32)
        lib.hydra_dkv(qkv, dout, wsp, dkv, scale, B, N, C, heads, dt)
        dqkv = torch.empty_like(qkv)
        dcv = torch.empty_like(cv)
        lib.hydra_apply_bwd(qkv, kv, dkv, cv, dout, dqkv, dcv, scale, B, N, C, heads, dt)
        return (dqkv, None, None, None, None) + _crpe_backward(qkv, dcv, dqkv, H, W, ctx.params)


def hydra_att(qkv, size, heads, scale, crpe_convs):
    """qkv [B,N,3C] tokens, size = (H, W), crpe_convs = the nn.Conv2d list of ConvRelPosEnc (windows 3/5/7 over head splits)"""
    return _HydraAtt.apply(qkv, int(size[0]), int(size[1]), int(heads), float(scale), *_crpe_wb(crpe_convs))


class _MaxPool2(_FastFunction):
    @staticmethod
    def forward(ctx, x, fork=False):
        """fork: also return an alias of x, which is what the OTHER consumers of x read, so that in the backward pass their gradient arrives here and is
        added inside the pooling scatter kernel (tcct_maxpool2_bwd_add; autograd would otherwise run an accumulation pass)"""
        if fork:
            ctx.set_materialize_grads(False)      # an unused output must arrive as None in backward(), not as a zero-filled tensor
        _chk(x)
        N, H, W, C = x.shape
        y = torch.empty((N, H // 2, W // 2, C), device=x.device, dtype=x.dtype)
        lib.maxpool2_fwd(x, y, N, H, W, C, dtype_code(x.dtype))
        ctx.save_for_backward(x)
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        (x,) = ctx.saved_tensors
        N, H, W, C = x.shape
        if dy is None:
            return dskip, None
        dy = _as(dy, x.dtype)
        dx = torch.empty_like(x)
        if dskip is None:
            lib.maxpool2_bwd(x, dy, dx, N, H, W, C, dtype_code(x.dtype))
        else:
            lib.maxpool2_bwd_add(x, dy, _as(dskip, x.dtype), dx, N, H, W, C, dtype_code(x.dtype))
        return dx, None


def maxpool2(x):
    return _MaxPool2.apply(x, False)


def maxpool2_fork(x):
    """(maxpool2(x), x'): use x' (an alias of x) for every other consumer of x; see _MaxPool2.forward `fork`"""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return maxpool2(x), x
    return _MaxPool2.apply(x, True)


class _Bilinear(_FastFunction):
    @staticmethod
    def forward(ctx, x, Ho, Wo, align, res=None):
        _chk(x)
        N, H, W, C = x.shape
        y = torch.empty((N, Ho, Wo, C), device=x.device, dtype=x.dtype)
        if res is not None:
            _chk(res)
            if tuple(res.shape) != (N, Ho, Wo, C) or res.dtype != x.dtype:
                raise TcctError('bilinear: residual must have the output shape and the input dtype')
            lib.bilinear_add_fwd(x, res, y, N, H, W, C, Ho, Wo, int(align), dtype_code(x.dtype))
        else:
            lib.bilinear_fwd(x, y, N, H, W, C, Ho, Wo, int(align), dtype_code(x.dtype))
        ctx.cfg = (N, H, W, C, Ho, Wo, int(align))
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C, Ho, Wo, align = ctx.cfg
        dy = _c(dy)
        dx = torch.empty((N, H, W, C), device=dy.device, dtype=dy.dtype)
        if dy.dtype == torch.float32 and C % 4 != 0 and Ho >= 4 * H and Wo >= 4 * W and (2 * Wo) // W + 3 <= 40 and Wo * C * 4 <= 65536:
            # narrow fp32 maps enlarged >= 4x (the coarse aux logits): separable transpose, one coalesced pass over dy (x8: 0.28 -> 0.08 ms;
            # at x2 the 2-D table gather is still faster)
            ws = torch.empty(N * Ho * W * C, device=dy.device, dtype=torch.float32)
            lib.bilinear_bwd_separable(dy, dx, ws, N, H, W, C, Ho, Wo, align)
        else:
            lib.bilinear_bwd(dy, dx, N, H, W, C, Ho, Wo, align, dtype_code(dy.dtype))
        return dx, None, None, None, (dy if ctx.has_res else None)


def bilinear(x, size, align_corners, residual=None):
    """F.interpolate(mode='bilinear') on NHWC; residual (output-shaped) is added in the same pass (decoder skip connections)"""
    if tuple(x.shape[1:3]) == tuple(size):
        return x if residual is None else add(x, residual)      # identity resize (torch returns the same values)
    return _Bilinear.apply(x, int(size[0]), int(size[1]), bool(align_corners), residual)


class _L2Norm(_FastFunction):
    @staticmethod
    def forward(ctx, x, eps):
        _chk(x)
        C = x.shape[-1]
        y = torch.empty_like(x)
        lib.l2norm_fwd(x, y, x.numel() // C, C, eps, dtype_code(x.dtype))
        ctx.save_for_backward(x)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _as(dy, x.dtype)
        C = x.shape[-1]
        dx = torch.empty_like(x)
        lib.l2norm_bwd(x, dy, dx, x.numel() // C, C, ctx.eps, dtype_code(x.dtype))
        return dx, None


def l2norm(x, eps=1e-12):
    return _L2Norm.apply(x, float(eps))


# ---- the feature-polarization gradient without its tensor (round 4) ---------------------------------------------------------------------------
# regular_udh's d loss / d feats is g * dpro[label[p]][bin[p]] -- a table lookup by two bytes per pixel.  When feats comes out of the fused norm_add
# node and the FPL is its only differentiable consumer (how FTC / RegNet use it), _Fpl.backward files (labels, binmap, table, upstream gradient, n_class)
# on the node's LazyGrad link and returns the placeholder; _NormAdd.backward takes the recipe and runs the lookup forms of its three kernels
# (tcct_l2norm_bwd_fplgrad, tcct_bilinear_bwd_fplgrad): the 452 MB gradient (bench shape) is neither written nor read three times.  With a second
# differentiable consumer of feats, or the FPL evaluated twice on the same feats, the node materialises the recipes (tcct_fpl_backward) and adds them.  A feats
# tensor with hooks / retain_grad (somebody wants to SEE the gradient) never takes the lazy path.  `FPL_LAZY_GRAD = False` (bench.py --set FPL_LAZY_GRAD=0) restores the dense tensor everywhere.
FPL_LAZY_GRAD = True


def _fpl_materialise(dc):
    """materialise(recipe, out) of _add_materialised for the recipes _Fpl.backward files"""
    return lambda r, d: lib.fpl_backward(r[1], r[2], r[3], r[4], 1.0, int(r[1].numel()), d, dc)


class _NormAdd(_FastFunction):
    """norm_add([g0, g1, g2]) (reference nets/tcct.py:937-942): mean of the three L2-normalised maps at g0's size.  Forward: one pass
    (tcct_normadd_fwd); backward: the existing resize / normalise gradients with the 1/3 folded into the last kernel of each chain."""

    @staticmethod
    def forward(ctx, g0, g1, g2, eps, fork=False):
        """fork: also return aliases of g0 / g1 / g2 for their other consumers (the aux heads); the gradients those deliver are added inside this
        node's last backward kernels (tcct_l2norm_bwd_scaled_add) instead of by three autograd accumulation passes"""
        ctx.set_materialize_grads(False)
        _chk(g0, g1, g2)
        N, H, W, C = g0.shape
        (_, h1, w1, _), (_, h2, w2, _) = g1.shape, g2.shape
        out = torch.empty_like(g0)
        inv1 = torch.empty(N * h1 * w1, device=g0.device, dtype=torch.float32)
        inv2 = torch.empty(N * h2 * w2, device=g0.device, dtype=torch.float32)
        lib.normadd_fwd(g0, g1, g2, inv1, inv2, out, N, H, W, C, h1, w1, h2, w2, eps, dtype_code(g0.dtype))
        ctx.save_for_backward(g0, g1, g2)
        ctx.eps = eps
        ctx.link = LazyGrad()
        if fork and C == 32:
            ctx.link.register(out)
        return (out, g0.view_as(g0), g1.view_as(g1), g2.view_as(g2)) if fork else out

    @staticmethod
    def backward(ctx, dy, *dalias):
        g0, g1, g2 = ctx.saved_tensors
        dalias = tuple(dalias) + (None,) * (3 - len(dalias))
        lazy, rest = ctx.link.take(dy)          # recipes of every _Fpl node that consumed THIS node's output
        if dy is None and not rest:             # only the aliases were used downstream
            return dalias[0], dalias[1], dalias[2], None, None
        N, H, W, C = g0.shape
        dc = dtype_code(g0.dtype)
        if lazy is None:
            dy = _add_materialised(dy, rest, g0, _fpl_materialise(dc))
        else:                   # the gradient is the feature-polarization loss's: looked up, never materialised
            _, labels, binmap, dpro, gup, ncls = lazy
        outs = []
        for g, da in zip((g0, g1, g2), dalias):
            h, w = g.shape[1], g.shape[2]
            M = g.numel() // C
            d = torch.empty_like(g)
            da = _c(_as(da, g.dtype)) if da is not None else None
            if lazy is not None and (h, w) == (H, W):
                lib.l2norm_bwd_fplgrad(g, labels, binmap, dpro, gup, 1.0, ncls, da, d, M, ctx.eps, 1.0 / 3.0, dc)
            else:
                if (h, w) == (H, W):
                    dn = dy
                else:
                    dn = torch.empty_like(g)
                    if lazy is not None:
                        lib.bilinear_bwd_fplgrad(labels, binmap, dpro, gup, 1.0, ncls, dn, N, h, w, H, W, 0, dc)
                    else:
                        lib.bilinear_bwd(dy, dn, N, h, w, C, H, W, 0, dc)
                if da is not None:
                    lib.l2norm_bwd_scaled_add(g, dn, da, d, M, C, ctx.eps, 1.0 / 3.0, dc)
                else:
                    lib.l2norm_bwd_scaled(g, dn, d, M, C, ctx.eps, 1.0 / 3.0, dc)
            outs.append(d)
        return outs[0], outs[1], outs[2], None, None


def _norm_add3_ok(g0, g1, g2):
    """the shapes _NormAdd takes: three NHWC maps of one dtype and channel count (C % 4 == 0, C/4 a power of two <= 64), g1 / g2 not at g0's size"""
    C = g0.shape[-1]
    lp = C // 4
    return (g0.dim() == 4 and g1.shape[-1] == C and g2.shape[-1] == C and C % 4 == 0 and 1 <= lp <= 64 and lp & (lp - 1) == 0
            and g0.dtype == g1.dtype == g2.dtype and tuple(g1.shape[1:3]) != tuple(g0.shape[1:3]) and tuple(g2.shape[1:3]) != tuple(g0.shape[1:3]))


def norm_add3(g0, g1, g2, eps=1e-12):
    """fused norm_add for three maps with the same channel count (C % 4 == 0, C/4 a power of two <= 64); g1 / g2 coarser than g0"""
    if not _norm_add3_ok(g0, g1, g2):
        size = tuple(g0.shape[1:3])
        return add3_scale(l2norm(g0, eps), bilinear(l2norm(g1, eps), size, False), bilinear(l2norm(g2, eps), size, False), 1.0 / 3.0)
    return _NormAdd.apply(g0, g1, g2, float(eps))


def norm_add3_fork(g0, g1, g2, eps=1e-12):
    """(norm_add3(g0, g1, g2), g0', g1', g2'): the aliases are to be read by the other consumers of the three maps (the aux heads); returns None
    when the fused form does not apply (the caller then uses norm_add3 and lets autograd accumulate)"""
    if not (_norm_add3_ok(g0, g1, g2) and torch.is_grad_enabled()):
        return None
    return _NormAdd.apply(g0, g1, g2, float(eps), True)


class _NormAdd6(_FastFunction):
    """norm_add([x1, x2, x3, y0, y1, y2]) of the legacy head layout (reference task1/onnx/tcct_goals.py:944-947,1024): the mean of six L2-normalised
    maps, two per resolution.  Forward: one pass (tcct_normadd6_fwd; each coarse pair is normalised and added before its one resize).  Backward: the
    two maps of a level share their incoming gradient -- dy at level 0, ONE resize gradient per coarse level -- which tcct_l2norm_bwd2_scaled reads
    once for both, the 1/6 folded in.  Takes part in the lazy feature-polarization gradient exactly as _NormAdd does."""

    @staticmethod
    def forward(ctx, a0, b0, a1, b1, a2, b2, eps):
        ctx.set_materialize_grads(False)
        _chk(a0, b0, a1, b1, a2, b2)
        N, H, W, C = a0.shape
        (_, h1, w1, _), (_, h2, w2, _) = a1.shape, a2.shape
        out = torch.empty_like(a0)
        inv1 = torch.empty(2 * N * h1 * w1, device=a0.device, dtype=torch.float32)
        inv2 = torch.empty(2 * N * h2 * w2, device=a0.device, dtype=torch.float32)
        lib.normadd6_fwd(a0, b0, a1, b1, a2, b2, inv1, inv2, out, N, H, W, C, h1, w1, h2, w2, eps, dtype_code(a0.dtype))
        ctx.save_for_backward(a0, b0, a1, b1, a2, b2)
        ctx.eps = eps
        ctx.link = LazyGrad()
        ctx.link.register(out)
        return out

    @staticmethod
    def backward(ctx, dy):
        xs = ctx.saved_tensors
        a0 = xs[0]
        lazy, rest = ctx.link.take(dy)          # recipes of every _Fpl node that consumed THIS node's output
        if dy is None and not rest:
            return (None,) * 7
        N, H, W, C = a0.shape
        dc = dtype_code(a0.dtype)
        if lazy is None:
            dy = _add_materialised(dy, rest, a0, _fpl_materialise(dc))
        else:                   # the gradient is the feature-polarization loss's: looked up, never materialised
            _, labels, binmap, dpro, gup, ncls = lazy
        outs = []
        for a, b in ((xs[0], xs[1]), (xs[2], xs[3]), (xs[4], xs[5])):
            h, w = a.shape[1], a.shape[2]
            da, db = torch.empty_like(a), torch.empty_like(b)
            M = a.numel() // C
            if lazy is not None and (h, w) == (H, W):
                lib.l2norm_bwd2_fplgrad(a, b, labels, binmap, dpro, gup, 1.0, ncls, None, None, da, db, M, ctx.eps, 1.0 / 6.0, dc)
            else:
                if (h, w) == (H, W):
                    dn = dy
                else:                                       # ONE resize gradient for the pair
                    dn = torch.empty_like(a)
                    if lazy is not None:
                        lib.bilinear_bwd_fplgrad(labels, binmap, dpro, gup, 1.0, ncls, dn, N, h, w, H, W, 0, dc)
                    else:
                        lib.bilinear_bwd(dy, dn, N, h, w, C, H, W, 0, dc)
                lib.l2norm_bwd2_scaled(a, b, dn, None, None, da, db, M, C, ctx.eps, 1.0 / 6.0, dc)
            outs += [da, db]
        return (*outs, None)


def norm_add6_fused_ok(a0, b0, a1, b1, a2, b2):
    """the shapes tcct_normadd6_fwd covers: 32 channels, one dtype, the two maps of a level alike, levels at H, H/2, H/4 with H % 8 == 0"""
    ts = (a0, b0, a1, b1, a2, b2)
    if any(t.dim() != 4 or t.shape[-1] != 32 or t.dtype != a0.dtype or t.shape[0] != a0.shape[0] for t in ts):
        return False
    if a0.dtype not in (torch.float32, torch.bfloat16) or any(a.shape != b.shape for a, b in ((a0, b0), (a1, b1), (a2, b2))):
        return False
    H = a0.shape[1]
    return H % 8 == 0 and H == 2 * a1.shape[1] == 4 * a2.shape[1]


def norm_add6(a0, b0, a1, b1, a2, b2, eps=1e-12):
    """norm_add of six maps, two per level (a_i, b_i alike; levels 1 / 2 coarser than level 0): the `feats` of the legacy head layout (reference
    task1/onnx/tcct_goals.py:1024, in its order [x1, x2, x3, y0, y1, y2] = [a0, a1, a2, b0, b1, b2]).  Fused for 32 channels at H, H/2, H/4 with
    H % 8 == 0; every other case is composed from l2norm / add / bilinear (the same values up to round-off)."""
    if norm_add6_fused_ok(a0, b0, a1, b1, a2, b2):
        return _NormAdd6.apply(a0, b0, a1, b1, a2, b2, float(eps))
    dt, size = a0.dtype, tuple(a0.shape[1:3])
    pair = [add(l2norm(_as(a, dt), eps), l2norm(_as(b, dt), eps)) for a, b in ((a0, b0), (a1, b1), (a2, b2))]
    return add3_scale(pair[0], bilinear(pair[1], size, False), bilinear(pair[2], size, False), 1.0 / 6.0)


# ------------------------------------------------------------------------------------------------ losses
# Three criterion families run the same three nodes (full resolution, upsampled head, deep supervision) over their own kernels:
#   'dice'   MultiLoss(DiceLoss), the benchmark's path               tcct_softmax_dice_*,  tcct_updice_*,  tcct_dice_ds_fwd    (csrc/loss.hip)
#   'crit'   MultiLoss dice / dice2 / iou / mse + class weights      tcct_softmax_crit_*,  tcct_upcrit_*,  tcct_crit_ds_fwd    (csrc/crit.hip)
#   'mcrit'  get_mloss per-sample dice / dice2 / iou, cross-entropy  tcct_softmax_mcrit_*, tcct_upmcrit_*, tcct_mcrit_ds_fwd   (csrc/mcrit.hip)
class _LossFamily:
    """What the families differ in on this side of the C-ABI.  Everything is fixed when the record is made, except the entry points themselves: the library loads lazily,
    so `fwd`, `bwd`, `up_fwd`, `up_bwd`, `ds_fwd` are bound on first use and are plain attributes from then on (what `lib.<name>` itself does)."""

    def __init__(self, tag, n_extra, per_sample):
        self.names = {'fwd': f'softmax_{tag}_fwd', 'bwd': f'softmax_{tag}_bwd', 'up_fwd': f'up{tag}_fwd', 'up_bwd': f'up{tag}_bwd', 'ds_fwd': f'{tag}_ds_fwd'}
        self.n_extra = n_extra                      # 2: (kind code, class_w) follow C in every call and the node's own arguments in `apply`; 0: Dice has neither
        if per_sample:                              # sums of a head fp64 [B][3][C], the full-resolution entry points take (B, HW)
            self.per_head, self.lead = (lambda B, C: B * 3 * C), (lambda B, n: (B, n // B))
        else:                                       # sums of a head fp64 [3][C], the full-resolution entry points take M = B * HW
            self.per_head, self.lead = (lambda B, C: 3 * C), (lambda B, n: (n,))

    def __getattr__(self, name):
        fn = getattr(lib, self.names[name])
        self.__dict__[name] = fn
        return fn


def _softmax_node(name, fam, doc=None):
    """<criterion>(logits NHWC [B,..,C], labels uint8): apply(logits, labels, *extra)"""
    nones = (None,) * (1 + fam.n_extra)

    def forward(ctx, logits, labels, *extra):
        _chk(logits, labels)
        B, C = logits.shape[0], logits.shape[-1]
        sums = torch.empty(fam.per_head(B, C), device=logits.device, dtype=torch.float64)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        fam.fwd(logits, labels, *fam.lead(B, logits.numel() // C), C, *extra, sums, loss, dtype_code(logits.dtype))
        ctx.save_for_backward(logits, labels, sums)
        ctx.cfg = extra
        return loss

    def backward(ctx, g):
        logits, labels, sums = ctx.saved_tensors
        B, C = logits.shape[0], logits.shape[-1]
        g = _as(g, torch.float32)
        d = torch.empty_like(logits)
        fam.bwd(logits, labels, *fam.lead(B, logits.numel() // C), C, *ctx.cfg, sums, g, 1.0, d, dtype_code(logits.dtype))
        return (d,) + nones

    return type(name, (_FastFunction,), {'forward': staticmethod(forward), 'backward': staticmethod(backward), '__doc__': doc})


def _upsampled_node(name, fam, doc):
    """<criterion>(F.interpolate(low, (H, W), 'bilinear'), labels) without materialising the resized logits (deep-supervision heads): apply(low, labels, H, W, *extra)"""
    nones = (None,) * (3 + fam.n_extra)

    def forward(ctx, low, labels, H, W, *extra):
        _chk(low, labels)
        B, h, w, C = low.shape
        sums = torch.empty(fam.per_head(B, C), device=low.device, dtype=torch.float64)
        loss = torch.empty((), device=low.device, dtype=torch.float32)
        fam.up_fwd(low, labels, B, h, w, H, W, C, *extra, sums, loss)
        ctx.save_for_backward(low, labels, sums)
        ctx.cfg = (H, W, extra)
        return loss

    def backward(ctx, g):
        low, labels, sums = ctx.saved_tensors
        B, h, w, C = low.shape
        H, W, extra = ctx.cfg
        g = _as(g, torch.float32)
        ws = torch.empty((B, H, w, C), device=low.device, dtype=torch.float32)
        d = torch.empty_like(low)
        fam.up_bwd(low, labels, B, h, w, H, W, C, *extra, sums, g, 1.0, ws, d)
        return (d,) + nones

    return type(name, (_FastFunction,), {'forward': staticmethod(forward), 'backward': staticmethod(backward), '__doc__': doc})


def _deep_supervision_node(name, fam, doc):
    """sum_{i = n..1} coff * <criterion>(resize(low_i)) + <criterion>(logits0) as ONE node: apply(logits0, labels, coff, H, W, *extra, *lows).  sums: head i at
    [i * per_head, (i + 1) * per_head), head 0 = the full-resolution one; the backward kernels of the low-resolution heads take coff as their grad_scale."""
    n_extra = fam.n_extra
    nones = (None,) * (4 + n_extra)

    def forward(ctx, logits0, labels, coff, H, W, *rest):
        extra, lows = rest[:n_extra], rest[n_extra:]
        _chk(logits0, labels, *lows)
        B, _, _, C = logits0.shape
        sums = torch.empty(4 * fam.per_head(B, C), device=logits0.device, dtype=torch.float64)
        loss = torch.empty((), device=logits0.device, dtype=torch.float32)
        a = []
        for i in range(3):
            a += [lows[i], lows[i].shape[1], lows[i].shape[2]] if i < len(lows) else [None, 0, 0]
        fam.ds_fwd(logits0, dtype_code(logits0.dtype), labels, B, H, W, C, *a, coff, *extra, sums, loss)
        ctx.save_for_backward(logits0, labels, sums, *lows)
        ctx.cfg = (coff, H, W, extra)
        return loss

    def backward(ctx, g):
        logits0, labels, sums, *lows = ctx.saved_tensors
        coff, H, W, extra = ctx.cfg
        B, _, _, C = logits0.shape
        per = fam.per_head(B, C)
        g = _as(g, torch.float32)
        d0 = torch.empty_like(logits0)
        fam.bwd(logits0, labels, *fam.lead(B, logits0.numel() // C), C, *extra, sums[:per], g, 1.0, d0, dtype_code(logits0.dtype))
        dl = []
        for i, low in enumerate(lows):
            _, h, w, _ = low.shape
            ws = torch.empty((B, H, w, C), device=low.device, dtype=torch.float32)
            d = torch.empty_like(low)
            fam.up_bwd(low, labels, B, h, w, H, W, C, *extra, sums[(i + 1) * per:(i + 2) * per], g, coff, ws, d)
            dl.append(d)
        return (d0,) + nones + tuple(dl)

    return type(name, (_FastFunction,), {'forward': staticmethod(forward), 'backward': staticmethod(backward), '__doc__': doc})


_DICE, _CRIT, _MCRIT = _LossFamily('dice', 0, False), _LossFamily('crit', 2, False), _LossFamily('mcrit', 2, True)

_SoftmaxDice = _softmax_node('_SoftmaxDice', _DICE)
_UpDice = _upsampled_node('_UpDice', _DICE, """MultiLoss(DiceLoss)(F.interpolate(low, size, 'bilinear'), labels) without materialising the resized logits (deep-supervision heads)""")
_DeepSupervisionDice = _deep_supervision_node('_DeepSupervisionDice', _DICE, """KiteSeg.grad_calc with MultiLoss(DiceLoss) (reference kite/loopback.py:62-73):
    sum_{i=3,2,1} coff * Dice(resize(low_i)) + Dice(logits0) as ONE node: one memset, four sums kernels, one finalisation; the scalar multiplications and additions of the
    loop (a dozen 5-us launches on the single-stream stretch of the step, each way) are arithmetic inside the finalisation kernel / the grad_scale argument of the backward
    kernels.""")
_SoftmaxCrit = _softmax_node('_SoftmaxCrit', _CRIT)
_UpCrit = _upsampled_node('_UpCrit', _CRIT, """MultiLoss(<kind>, weight)(F.interpolate(low, size, 'bilinear'), labels) without materialising the resized logits""")
_DeepSupervisionCrit = _deep_supervision_node('_DeepSupervisionCrit', _CRIT, """_DeepSupervisionDice for every criterion kind / class weights: one memset, up to four sums kernels,
    one finalisation""")
_SoftmaxMCrit = _softmax_node('_SoftmaxMCrit', _MCRIT)
_UpMCrit = _upsampled_node('_UpMCrit', _MCRIT, """<m-criterion>(F.interpolate(low, size, 'bilinear'), labels) without materialising the resized logits""")
_DeepSupervisionMCrit = _deep_supervision_node('_DeepSupervisionMCrit', _MCRIT, """_DeepSupervisionCrit for the m-criteria: one memset, up to four sums kernels, one finalisation""")


def softmax_dice(logits, labels):
    """MultiLoss(DiceLoss): logits NHWC [N,H,W,C], labels uint8 [N,H,W] -> scalar (sum over classes of 1-dice)."""
    return _SoftmaxDice.apply(logits, labels)


# The criterion family of the reference's MultiLoss (kite/losses/loss.py:9-110): per-class loss `kind` + per-class weights.  kind 'dice' without weights IS the Dice
# family (the benchmark's path, untouched); everything else runs the tcct_softmax_crit_* / tcct_upcrit_* / tcct_crit_ds_fwd kernels (csrc/crit.hip).
CRIT_KINDS = {'dice': 0, 'dice2': 1, 'iou': 2, 'mse': 3}
# The criteria of the reference's get_mloss (kite/losses/lossm.py over kite/losses/miou.py): Dice / dice2 / IoU taken per SAMPLE and per class, and
# nn.CrossEntropyLoss(weight) -- tcct_softmax_mcrit_* / tcct_upmcrit_* / tcct_mcrit_ds_fwd (csrc/mcrit.hip).  sums fp64 [head][B][3][C].
MCRIT_KINDS = {'dice': 0, 'dice2': 1, 'iou': 2, 'ce': 3}


def _class_w_ok(class_w, C, device):
    """The weights are read by the kernels at run time (a persistent buffer of the caller: graph-capturable)."""
    if class_w is not None and not (torch.is_tensor(class_w) and class_w.dtype == torch.float32 and class_w.dim() == 1 and class_w.numel() >= C
                                    and class_w.is_contiguous() and class_w.device == device):
        raise TcctError(f'class weights: a contiguous fp32 vector of at least {C} entries on {device} is needed')
    return class_w


def _crit_args(kind, class_w, C, device):
    """-> (kind code, fp32 [C] weights on `device` or None)"""
    if kind not in CRIT_KINDS:
        raise TcctError(f'criterion kind {kind!r}: one of {sorted(CRIT_KINDS)}')
    return CRIT_KINDS[kind], _class_w_ok(class_w, C, device)


def _mcrit_args(kind, class_w, C, device):
    """-> (kind code, class_w).  Only 'ce' takes class weights: the reference's MDiceLoss / MIouLoss have none."""
    if kind not in MCRIT_KINDS:
        raise TcctError(f'm-criterion kind {kind!r}: one of {sorted(MCRIT_KINDS)}')
    if class_w is not None and kind != 'ce':
        raise TcctError(f'm-criterion kind {kind!r} takes no class weights (only \'ce\' does)')
    return MCRIT_KINDS[kind], _class_w_ok(class_w, C, device)


def softmax_criterion(logits, labels, kind='dice', class_w=None):
    """MultiLoss(<kind>, weight): logits NHWC [N,H,W,C], labels uint8 [N,H,W] -> scalar sum_c class_w[c] * L_c.  kind: 'dice' | 'dice2' | 'iou' | 'mse' (the latter is
    nn.MSELoss against the FLOAT one-hot, per class a mean over all N*H*W pixels); class_w: fp32 device vector [>= C] or None (all ones)."""
    if kind == 'dice' and class_w is None:
        return _SoftmaxDice.apply(logits, labels)
    code, class_w = _crit_args(kind, class_w, logits.shape[-1], logits.device)
    return _SoftmaxCrit.apply(logits, labels, code, class_w)


def softmax_criterion_upsampled(lr, labels, kind='dice', class_w=None):
    """the criterion of a LowResLogits head"""
    if kind == 'dice' and class_w is None:
        return softmax_dice_upsampled(lr, labels)
    if not lr.fusable():
        return softmax_criterion(bilinear(lr.low, lr.size, False), labels, kind, class_w)
    code, class_w = _crit_args(kind, class_w, lr.low.shape[-1], lr.low.device)
    return _UpCrit.apply(lr.low, labels, lr.size[0], lr.size[1], code, class_w)


def deep_supervision_criterion(logits0_nhwc, labels, lows, coff, kind='dice', class_w=None):
    """deep_supervision_dice for every kind / class weights (same gate: deep_supervision_dice_ok)"""
    if kind == 'dice' and class_w is None:
        return deep_supervision_dice(logits0_nhwc, labels, lows, coff)
    code, class_w = _crit_args(kind, class_w, logits0_nhwc.shape[-1], logits0_nhwc.device)
    H, W = lows[0].size
    return _DeepSupervisionCrit.apply(logits0_nhwc, labels, float(coff), H, W, code, class_w, *[l_.low for l_ in lows])


def softmax_mcriterion(logits, labels, kind, class_w=None):
    """MDiceLoss(bi=False / True), MIouLoss, nn.CrossEntropyLoss(weight): logits NHWC [N,H,W,C], labels uint8 [N,H,W] -> scalar.  kind: 'dice' | 'dice2' | 'iou' (per
    sample and class, mean over N*C) | 'ce' (weighted mean over the pixels); class_w: fp32 device vector [>= C] or None, 'ce' only."""
    code, class_w = _mcrit_args(kind, class_w, logits.shape[-1], logits.device)
    return _SoftmaxMCrit.apply(logits, labels, code, class_w)


def softmax_mcriterion_upsampled(lr, labels, kind, class_w=None):
    """the m-criterion of a LowResLogits head"""
    if not lr.fusable():
        return softmax_mcriterion(bilinear(lr.low, lr.size, False), labels, kind, class_w)
    code, class_w = _mcrit_args(kind, class_w, lr.low.shape[-1], lr.low.device)
    return _UpMCrit.apply(lr.low, labels, lr.size[0], lr.size[1], code, class_w)


def deep_supervision_mcriterion(logits0_nhwc, labels, lows, coff, kind, class_w=None):
    """deep_supervision_criterion for the m-criteria (same gate: deep_supervision_dice_ok)"""
    code, class_w = _mcrit_args(kind, class_w, logits0_nhwc.shape[-1], logits0_nhwc.device)
    H, W = lows[0].size
    return _DeepSupervisionMCrit.apply(logits0_nhwc, labels, float(coff), H, W, code, class_w, *[l_.low for l_ in lows])


DS_DICE_FUSE = True        # False: one criterion node per head + torch scalar arithmetic (A/B timing)


def deep_supervision_dice_ok(outs, coff):
    """outs = [logits0 (NCHW view of NHWC memory or NHWC), LowResLogits x 1..3]"""
    return (DS_DICE_FUSE and isinstance(outs, (list, tuple)) and 2 <= len(outs) <= 4 and all(isinstance(o, LowResLogits) and o.fusable() for o in outs[1:])
            and torch.is_tensor(outs[0]) and outs[0].dim() == 4 and len({o.size for o in outs[1:]}) == 1)


def deep_supervision_dice(logits0_nhwc, labels, lows, coff):
    """sum_{i = n..1} coff * Dice(resize(lows[i-1])) + Dice(logits0): lows = [LowResLogits of outs[1], outs[2], ...] (the reference's loop runs from the last)"""
    H, W = lows[0].size
    return _DeepSupervisionDice.apply(logits0_nhwc, labels, float(coff), H, W, *[l_.low for l_ in lows])


# The HIP runtime multiplexes its streams onto FOUR hardware queues (GPU_MAX_HW_QUEUES; measured on the bench step: 3 queues 21.2 ms, 4 queues 20.26, 5 or more 24.6):
# streams beyond the fourth share a queue with another one and serialise against it.  The step therefore uses exactly four streams -- current, 'vit', 'vit_enc',
# 'wgrad' -- and the later forks REUSE the encoder streams, which are idle when the fusion / the losses run (forward: joined; backward: not started yet).
FUSE_STREAM_TAG = 'vit_enc'
REG_FORK = True          # RegNet.regular_reg: the `true` chain on the (idle) 'vit' stream beside the `pred` chain
LOSS_FORK = True         # KiteSeg.calc_loss: the boundary-regression loss on the (idle) 'vit_enc' stream beside Dice + feature polarization


def loss_fork_ok(logits):
    return (LOSS_FORK and STAGE_FORK_MAX_PIXELS > 0 and PARALLEL_BRANCHES and torch.is_grad_enabled() and logits.is_cuda and logits.requires_grad
            and logits.shape[0] * logits.shape[2] * logits.shape[3] >= (1 << 20))


class LowResLogits:
    """A deep-supervision head before its resize: `low` fp32 NHWC [B,h,w,C] + the target size.  FTC.forward returns these instead of
    the resized tensors when `defer_aux_resize` is set (KiteSeg.calc_loss does, in training); the Dice criterion consumes them with the
    fused resize + softmax + Dice kernels, anything else calls `.dense()` for the reference's [B,C,H,W] tensor."""

    def __init__(self, low, size):
        self.low, self.size = low, (int(size[0]), int(size[1]))

    def fusable(self):
        B, h, w, C = self.low.shape
        H, W = self.size
        return (self.low.dtype == torch.float32 and 2 <= C <= 8 and H % h == 0 and W % w == 0 and H // h == W // w and H // h in (2, 4, 8, 16))

    def dense(self):
        return bilinear(self.low, self.size, False).permute(0, 3, 1, 2)


def softmax_dice_upsampled(lr, labels):
    """Dice criterion of a LowResLogits head"""
    if not lr.fusable():
        return softmax_dice(bilinear(lr.low, lr.size, False), labels)
    return _UpDice.apply(lr.low, labels, lr.size[0], lr.size[1])


class _Slice(_FastFunction):
    @staticmethod
    def forward(ctx, x, start, n):
        _chk(x)
        C = x.shape[-1]
        M = x.numel() // C
        y = torch.empty(x.shape[:-1] + (n,), device=x.device, dtype=torch.float32)
        lib.slice_channels_fwd(x, y, M, C, start, n, dtype_code(x.dtype))
        ctx.cfg = (C, start, n, x.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        C, start, n, dt = ctx.cfg
        dy = _as(dy, torch.float32)
        M = dy.numel() // n
        dx = torch.empty(dy.shape[:-1] + (C,), device=dy.device, dtype=dt)
        lib.slice_channels_bwd(dy, dx, M, C, start, n, dtype_code(dt))
        return dx, None, None


def slice_channels_f32(x, start, n):
    return _Slice.apply(x, start, n)


class _GumbelColSoftmax(_FastFunction):
    @staticmethod
    def forward(ctx, x, eps):
        _chk(x, eps)
        N, H, W, CH = x.shape
        out = torch.empty((N, H, W, 1), device=x.device, dtype=torch.float32)
        stats = torch.empty((N, W, CH, 3), device=x.device, dtype=torch.float32)
        lib.gumbel_colsoftmax_fwd(x, eps, out, stats, N, H, W, CH)
        ctx.save_for_backward(x, eps, stats)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, eps, stats = ctx.saved_tensors
        N, H, W, CH = x.shape
        dout = _as(dout, torch.float32)
        dx = torch.empty_like(x)
        lib.gumbel_colsoftmax_bwd(x, eps, stats, dout, dx, N, H, W, CH)
        return dx, None


def gumbel_colsoftmax_sum(x, eps):
    """x, eps fp32 [N,H,W,4] -> [N,H,W,1]: sum_c sampling_softmax over H (reg.py:118-128)"""
    return _GumbelColSoftmax.apply(x, eps)


class _ColSoftmax(_FastFunction):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        N, H, W = x.shape[:3]
        y = torch.empty_like(x)
        lib.colsoftmax_fwd(x, y, N, H, W)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        N, H, W = y.shape[:3]
        dy = _as(dy, torch.float32)
        dx = torch.empty_like(y)
        lib.colsoftmax_bwd(y, dy, dx, N, H, W)
        return dx


def colsoftmax(x):
    """softmax over H of fp32 [N,H,W,1]"""
    return _ColSoftmax.apply(x)


class _ColWSum(_FastFunction):
    @staticmethod
    def forward(ctx, x, wts):
        _chk(x, wts)
        N, H, W = x.shape[:3]
        out = torch.empty((N, W), device=x.device, dtype=torch.float32)
        lib.colwsum_fwd(x, wts, out, N, H, W)
        ctx.save_for_backward(wts)
        ctx.shape = x.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        (wts,) = ctx.saved_tensors
        N, H, W = ctx.shape[:3]
        dout = _as(dout, torch.float32)
        dx = torch.empty(ctx.shape, device=dout.device, dtype=torch.float32)
        lib.colwsum_bwd(dout, wts, dx, N, H, W)
        return dx, None


def colwsum(x, wts):
    """edge[n,w] = sum_h x[n,h,w]*wts[h]"""
    return _ColWSum.apply(x, wts)


class _Mse(_FastFunction):
    @staticmethod
    def forward(ctx, a, b):
        _chk(a, b)
        acc = torch.empty((), device=a.device, dtype=torch.float64)
        out = torch.empty((), device=a.device, dtype=torch.float32)
        lib.mse_fwd(a, b, a.numel(), acc, out)
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _as(g, torch.float32)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        lib.mse_bwd(a, b, a.numel(), g, 1.0, da, db)
        return da, db


def mse(a, b):
    return _Mse.apply(a, b)


def label_planes(labels, start, n, want_onehot=True, want_edge=True):
    """labels uint8 [N,H,W] -> (onehot fp32 [N,H,W,n] of classes start.., edge fp32 [N,H,W,1])"""
    _chk(labels)
    N, H, W = labels.shape
    oh = torch.empty((N, H, W, n), device=labels.device, dtype=torch.float32) if want_onehot else None
    ed = torch.empty((N, H, W, 1), device=labels.device, dtype=torch.float32) if want_edge else None
    lib.label_planes(labels, oh, ed, N, H, W, start, n)
    return oh, ed


class _Fpl(_FastFunction):
    @staticmethod
    def forward(ctx, feat, logits, labels, buf_grad, allow_lazy=True):
        ctx.set_materialize_grads(False)      # an unused output must arrive as None in backward(), not as a zero-filled tensor
        _chk(feat, logits, labels, buf_grad)
        C = logits.shape[-1]
        M = logits.numel() // C
        dev = feat.device
        if feat.shape[-1] != 32:
            raise TcctError('fpl: feature width must be 32')
        prob = torch.empty(M, device=dev, dtype=torch.float32)
        lib.softmax_pick(logits, labels, M, C, prob, None, dtype_code(logits.dtype))
        counts = torch.empty(16, device=dev, dtype=torch.int32)        # FPL_MAXC
        pro_sum = torch.empty((C, 32, 32), device=dev, dtype=torch.float32)
        pro = torch.empty((C, 32, 32), device=dev, dtype=torch.float32)
        dpro = torch.empty((C, 32, 32), device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        binmap = torch.empty(M, device=dev, dtype=torch.uint8)
        # radix multi-select of the 32 bin boundaries per class + bin sums in pixel order (fpl_select.hip): no sort, no gather
        ws = torch.empty(int(lib.fpl_select_workspace_bytes()), device=dev, dtype=torch.uint8)
        lib.fpl_select(feat, labels, prob, M, C, ws, counts, binmap, pro_sum, dtype_code(feat.dtype))
        lib.fpl_loss(pro_sum, counts, buf_grad, C, pro, loss, dpro)
        ctx.save_for_backward(labels, binmap, dpro)
        ctx.cfg = (feat.shape, feat.dtype, M)
        # feat is the output of a norm_add node that can look its gradient up from (labels, bins, table) itself (FPL_LAZY_GRAD above): its link, else None
        ctx.lazy = LazyGrad.of(feat) if (FPL_LAZY_GRAD and allow_lazy and feat.shape[-1] == 32 and feat.is_contiguous()) else None
        ctx.mark_non_differentiable(pro)
        return loss, pro

    @staticmethod
    def backward(ctx, g, _gpro):
        labels, binmap, dpro = ctx.saved_tensors
        shape, dt, M = ctx.cfg
        if g is None:
            return None, None, None, None, None
        g = _as(g, torch.float32)
        if ctx.lazy is not None:
            # d loss / d feat is a function of two bytes per pixel: hand norm_add's backward the recipe instead of the 452 MB tensor
            return ctx.lazy.file((labels, binmap, dpro, g, int(dpro.shape[0])), shape, dt, g.device), None, None, None, None
        dfeat = torch.empty(shape, device=g.device, dtype=dt)
        lib.fpl_backward(labels, binmap, dpro, g, 1.0, M, dfeat, dtype_code(dt))
        return dfeat, None, None, None, None


def grad_is_watched(t):
    """somebody hooks `t` or retains its gradient, i.e. wants to SEE d loss / d t: such a tensor never receives a recipe gradient.  Only what exists when the
    consumer's forward runs is visible here (the LIMITATION in LazyGrad's docstring)."""
    return bool(getattr(t, 'retains_grad', False)) or bool(getattr(t, '_backward_hooks', None))


def fpl(feat, logits, labels, buf_grad, allow_lazy=True):
    """regular_udh: feat NHWC [N,H,W,32], logits NHWC [N,H,W,C] (no grad flows to them), labels uint8 [N,H,W],
    buf_grad fp32 [C,32] -> (loss, prototypes [C,32,32]).  allow_lazy=False (or a watched `feat`): the gradient wrt feat is the dense tensor."""
    return _Fpl.apply(feat, logits.detach(), labels, buf_grad, bool(allow_lazy) and not grad_is_watched(feat))


# ---------------------------------------------------------------------------------------------------------------- layout likelihood loss
_LAYOUT_LABEL_CACHE = {}


def layout_label(labels_u8, layout, valid=None):
    """(t uint8 [B,H,W], bnd_lab int32 [B,S-1,W]) = mask and surfaces of `evalm.layout_decode` of the label under `layout`: the nearest label the layout can
    produce, what the evaluator scores against.  One-entry cache per label tensor, with the rules of `nets.reg.as_label_index`."""
    from . import evalm
    key = (labels_u8.data_ptr(), tuple(labels_u8.shape), labels_u8._version, layout, valid)
    hit = _LAYOUT_LABEL_CACHE.get('k')
    if hit is not None and hit[0] == key and hit[2]() is labels_u8:
        return hit[1]
    t, bnd = evalm.layout_decode(labels_u8, layout, valid)[:2]
    _LAYOUT_LABEL_CACHE['k'] = (key, (t, bnd), weakref.ref(labels_u8))
    return t, bnd


class _LayoutNll(_FastFunction):
    @staticmethod
    def forward(ctx, logits, t, bnd, layout, hv, wv, tau):
        B, H, W, C = logits.shape
        S, dev = layout.n_states, logits.device
        nbytes = lib.layout_nll_ws_bytes(B, H, W, S, len(layout.free))
        if nbytes < 0:
            raise TcctError(f'tcct_layout_nll_ws_bytes failed: {lib.last_error()}')
        ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)              # lives until backward: the upward walk reads what the downward walk left
        nll = torch.empty((B, W), device=dev, dtype=torch.float32)
        out = torch.empty((2,), device=dev, dtype=torch.float32)               # loss, 1 / N: both formed on the device
        kind = dtype_code(logits.dtype)
        lib.layout_nll_fwd(logits, kind, t, bnd, B, H, W, C, layout._c_layers, S, layout.free_mask, hv, wv, tau, ws, nll)
        lib.layout_nll_reduce(nll, bnd, B, S, W, hv, wv, out)
        ctx.save_for_backward(logits, t, bnd, ws, out)
        ctx.cfg = (layout, hv, wv, tau)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        logits, t, bnd, ws, out = ctx.saved_tensors
        layout, hv, wv, tau = ctx.cfg
        B, H, W, C = logits.shape
        gscale = (_as(g, torch.float32) * out[1]).reshape(1)                   # grad_output / N: one float, read by the kernel
        grad = torch.empty_like(logits)
        lib.layout_nll_bwd(logits, dtype_code(logits.dtype), t, bnd, B, H, W, C, layout._c_layers, layout.n_states, layout.free_mask, hv, wv, tau, ws, gscale, grad)
        return grad, None, None, None, None, None, None


def layout_nll(logits_nhwc, labels_u8, layout, valid=None, tau=1.0):
    """Layout likelihood loss (layout_loss.hip): the mean over the annotated columns and their h_valid rows of -log P(label | ordered), the share the
    label's (state sequence, shown classes) pair holds of the column's partition function of `evalm.layout_marginals`.  logits fp32 / bf16 NHWC [B,H,W,C];
    labels uint8 [B,H,W] (they go through `evalm.layout_decode` first: a label the layout cannot produce is replaced by the nearest one it can);
    valid = (h_valid, w_valid), default the whole image; tau > 0.  -> scalar fp32 tensor, 0 when no column is annotated; differentiable in the logits
    (the gradient is exact, in the logits' dtype).  Eager, on the current stream, no host sync; two calls give the same bits."""
    from . import evalm
    if not isinstance(layout, evalm.Layout):
        raise TcctError(f'layout_nll: layout must be an evalm.Layout, got {type(layout).__name__}')
    try:
        tau = float(tau)
    except (TypeError, ValueError):
        raise TcctError(f'layout_nll: tau={tau!r} (a positive temperature)')
    if not 0.0 < tau < float('inf'):
        raise TcctError(f'layout_nll: tau={tau!r} (a positive temperature)')
    if not (torch.is_tensor(logits_nhwc) and logits_nhwc.is_cuda and torch.is_tensor(labels_u8) and labels_u8.is_cuda):
        raise TcctError('layout_nll: logits and labels must be CUDA tensors (no CPU fallback)')
    if logits_nhwc.dtype not in (torch.float32, torch.bfloat16):
        raise TcctError(f'layout_nll: fp32 / bf16 logits [B,H,W,C] expected, got {logits_nhwc.dtype}')
    C = layout.n_class
    if logits_nhwc.dim() != 4 or logits_nhwc.shape[3] != C:
        raise TcctError(f'layout_nll: logits {tuple(logits_nhwc.shape)} are not NHWC [B,H,W,{C}]')
    B, H, W = logits_nhwc.shape[:3]
    if labels_u8.dtype != torch.uint8 or tuple(labels_u8.shape) != (B, H, W):
        raise TcctError(f'layout_nll: labels must be uint8 class indices [{B},{H},{W}], got {labels_u8.dtype}{tuple(labels_u8.shape)}')
    hv, wv = (H, W) if valid is None else (int(valid[0]), int(valid[1]))
    t, bnd = layout_label(labels_u8.contiguous(), layout, (hv, wv))
    return _LayoutNll.apply(logits_nhwc.contiguous(), t, bnd, layout, hv, wv, tau)
