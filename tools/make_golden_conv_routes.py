"""Records which C-ABI calls the convolution and pointwise nodes of tcct_amd.ops make -> tests/golden/conv_routes.json (tests/test_conv_routes_gpu.py
replays the same cases and compares call by call).  Needs the GPU.

    python tools/make_golden_conv_routes.py                       # writes the fixture
    python tools/make_golden_conv_routes.py --out /tmp/a.json     # somewhere else (record twice, compare)
    python tools/make_golden_conv_routes.py --steps-full /tmp/s   # also the full call sequences of the whole steps, one JSON file each, for diffing

Only `ops.*` entry points and the `tcct_amd._lib._TRACE` hook are used, so the script runs unchanged against any revision of ops.py: the fixture is recorded
at the revision whose behaviour is to be kept, not at the one under test.

Per call: the symbol and, in the order of the prototype, every non-pointer argument's value, for every pointer argument None or [dtype, shape] of the tensor
passed, and the stream as an index in order of first appearance within the case.  Pointer VALUES are not recorded.  The argument names of every symbol seen are
kept beside the calls (`symbols`), so a changed prototype shows as a difference too.  For the whole training / inference steps only the number of calls, the
count per symbol and a SHA-256 of the canonical sequence are kept.

The file stores the sequences losslessly but compactly (encode / decode below): a call is [symbol index, values] the first time its symbol appears in a case and
[symbol index, position, value, position, value, ...] -- what changed against the previous call of that symbol -- afterwards; a tensor is "dtype[shape]"; a
pooled case whose calls equal those of the case outside begin_step / end_step is stored as the string SAME; a changed integer is stored as its increment ("+32"), which makes the rounds of the slab loops equal entries, and ["*", n, [entries]]
stands for those entries n times in a row.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json')
BF, F32 = torch.bfloat16, torch.float32
_DT = {torch.bfloat16: 'bf16', torch.float32: 'f32', torch.float64: 'f64', torch.int64: 'i64', torch.int32: 'i32', torch.uint8: 'u8'}

# Cin_w, Cout, KH, KW, stride, ph, pw, H, W: the rows of tests/test_kernels_gpu.py::test_conv2d
CONV2D = [
    (32, 32, 3, 3, 1, 1, 1, 17, 23), (32, 32, 1, 13, 1, 0, 6, 9, 40), (32, 32, 13, 1, 1, 6, 0, 40, 9),
    (3, 32, 3, 3, 1, 1, 1, 16, 16), (3, 32, 3, 3, 2, 1, 1, 16, 20), (32, 64, 3, 3, 1, 1, 1, 8, 12),
    (128, 96, 1, 1, 1, 0, 0, 6, 10), (32, 5, 1, 1, 1, 0, 0, 12, 8), (320, 160, 1, 1, 1, 0, 0, 4, 6),
    (160, 32, 1, 1, 1, 0, 0, 4, 6), (32, 32, 3, 3, 1, 1, 1, 70, 130), (32, 32, 1, 11, 1, 0, 5, 20, 150),
    (32, 32, 9, 1, 1, 4, 0, 150, 20), (32, 32, 5, 1, 1, 2, 0, 64, 8), (32, 32, 1, 5, 1, 0, 2, 8, 64), (32, 32, 7, 1, 1, 3, 0, 33, 9),
    (32, 32, 1, 7, 1, 0, 3, 9, 33), (32, 32, 1, 1, 1, 0, 0, 19, 70), (64, 64, 1, 1, 1, 0, 0, 21, 33), (96, 32, 1, 1, 1, 0, 0, 9, 50),
    (192, 128, 1, 1, 1, 0, 0, 10, 17), (256, 160, 1, 1, 1, 0, 0, 7, 9), (64, 96, 1, 1, 1, 0, 0, 40, 55), (32, 64, 3, 3, 1, 1, 1, 19, 70), (64, 32, 3, 3, 1, 1, 1, 19, 70),
    (64, 64, 3, 3, 1, 1, 1, 9, 40),
    (32, 64, 1, 11, 1, 0, 5, 12, 40), (64, 64, 11, 1, 1, 5, 0, 40, 12), (64, 96, 1, 9, 1, 0, 4, 9, 33), (96, 96, 9, 1, 1, 4, 0, 33, 9),
    (96, 128, 3, 3, 1, 1, 1, 10, 14), (128, 128, 7, 1, 1, 3, 0, 20, 6), (128, 256, 1, 5, 1, 0, 2, 5, 9), (256, 256, 3, 3, 1, 1, 1, 4, 6),
    (256, 128, 3, 3, 1, 1, 1, 6, 8)]
# Cin, Cout, KH, KW, pre, H, W: the rows of test_convolutions_deliver_the_batchnorm_statistics_of_their_consumer
STATS = [(32, 64, 3, 3, 'none', 19, 70), (64, 96, 1, 9, 'lrelu', 9, 33), (96, 32, 3, 3, 'none', 10, 14), (32, 32, 3, 3, 'lrelu', 21, 37),
         (64, 64, 1, 1, 'none', 40, 55), (160, 160, 1, 1, 'none', 50, 69), (160, 160, 1, 1, 'none', 300, 240), (128, 160, 1, 1, 'none', 13, 9)]
# Cin, Cout, KH, KW, pre, post, has_bn, tokens: the rows of test_conv_bn_act_inference (N, H, W = 2, 19, 70)
INFER = [(64, 64, 1, 1, None, 'hswish', True, False), (32, 32, 3, 3, 'lrelu', None, True, False), (32, 32, 1, 13, None, 'lrelu', True, False),
         (96, 32, 1, 1, None, None, True, False), (64, 64, 1, 1, None, 'gelu', False, True), (128, 96, 1, 1, None, 'hswish', True, False),
         (32, 32, 13, 1, None, None, False, False), (32, 5, 1, 1, None, None, False, False)]
# dtype, Cin, Cout, k: conv2d_fork with both outputs used / one operand without requires_grad
FORK = [(BF, 32, 32, 3), (BF, 64, 64, 1), (BF, 32, 64, 3), (F32, 32, 32, 3)]


class Recorder:
    """the _TRACE hook: one [symbol, [argument values..., stream index]] per call"""

    def __init__(self):
        self.calls, self.symbols, self.streams = [], {}, {}

    def __call__(self, full, sig, args):
        vals = []
        for (ct, nm), a in zip(sig, args):
            if nm == 'stream':
                vals.append(self.streams.setdefault(a, len(self.streams)))
            elif ct is ctypes.c_void_p:
                if a is None:
                    vals.append(None)
                elif isinstance(a, torch.Tensor):
                    vals.append([_DT.get(a.dtype, str(a.dtype)), list(a.shape)])
                else:
                    vals.append('raw pointer')
            else:
                vals.append(a)
        self.symbols[full] = [nm for _, nm in sig]
        self.calls.append([full, vals])


def _record(fn):
    from tcct_amd import _lib
    rec = Recorder()
    prev, _lib._TRACE[0] = _lib._TRACE[0], rec
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib._TRACE[0] = prev
    return rec


def _t(*shape, dt=F32, grad=False):
    return torch.randn(*shape, device='cuda').to(dt).requires_grad_(grad)


def _bwd(outs):
    outs = [o for o in (outs if isinstance(outs, (tuple, list)) else [outs]) if o is not None]
    torch.autograd.backward(outs, [torch.randn(o.shape, device='cuda').to(o.dtype) for o in outs])


def _bn(C):
    return (1 + 0.3 * _t(C), 0.2 * _t(C), 0.5 * _t(C), 0.5 + _t(C).abs(), 1e-5)


def cases():
    """-> [(name, make)]: make() builds the operands once and returns the closure that runs forward + backward on them (the pack registry keys on the weight
    tensor, so the pooled variant has to run the same tensors twice)"""
    from tcct_amd import ops
    out = []

    def add(name, make):
        out.append((name, make))

    for dt in (F32, BF):
        for Cw, Co, KH, KW, s, ph, pw, H, W in CONV2D:
            def make(dt=dt, Cw=Cw, Co=Co, KH=KH, KW=KW, s=s, ph=ph, pw=pw, H=H, W=W):
                x = _t(2, H, W, (Cw + 3) // 4 * 4, dt=dt, grad=Cw % 4 == 0)
                w, b = _t(Co, Cw, KH, KW, grad=True), _t(Co, grad=True)
                return lambda: _bwd(ops.conv2d(x, w, b, stride=s, pad=(ph, pw)))
            add(f'conv2d {_DT[dt]} {Cw}->{Co} {KH}x{KW} s{s} {H}x{W}', make)

    def head():
        x, w, b = _t(2, 37, 53, 32, dt=BF, grad=True), _t(5, 32, 1, 1, grad=True), _t(5, grad=True)
        return lambda: _bwd(ops.conv2d(x, w, b, out_dtype=F32))
    add('head bf16->f32 32->5', head)

    def tokens():
        x, w, b = _t(2, 50, 64, dt=BF, grad=True), _t(192, 64, grad=True), _t(192, grad=True)
        return lambda: _bwd(ops.conv2d(x, w, b))
    add('tokens [2,50,64] 64->192', tokens)

    for dt, Ci, Co, k in FORK:
        for gx, gw in ((True, True), (False, True), (True, False)):
            def make(dt=dt, Ci=Ci, Co=Co, k=k, gx=gx, gw=gw):
                x = _t(2, 13, 22, Ci, dt=dt, grad=gx)
                w, b = _t(Co, Ci, k, k, grad=gw), _t(Co, grad=gw)
                if gx and gw:
                    return lambda: _bwd(ops.conv2d_fork(x, w, b, pad=k // 2))
                return lambda: _bwd(ops.conv2d(x, w, b, pad=k // 2))
            add(f'{"fork" if gx and gw else "conv2d"} {_DT[dt]} {Ci}->{Co} {k}x{k} grad x={gx} w={gw}', make)

    for Ci, Co, KH, KW, pre, H, W in STATS:
        def make(Ci=Ci, Co=Co, KH=KH, KW=KW, pre=pre, H=H, W=W):
            x, w, b = _t(2, H, W, Ci, dt=BF, grad=True), _t(Co, Ci, KH, KW, grad=True), _t(Co, grad=True)
            return lambda: _bwd(ops.conv2d(x, w, b, pad=(KH // 2, KW // 2), stats_pre=pre))
        add(f'stats_pre={pre} {Ci}->{Co} {KH}x{KW} {H}x{W}', make)

    for C in (64, 160):
        for scaled in (False, True):
            def make(C=C, scaled=scaled):
                x, res = _t(3, 230, C, dt=BF, grad=True), _t(3, 230, C, dt=BF, grad=True)
                w, b = _t(C, C, grad=True), _t(C, grad=True)
                sc = torch.tensor([1.25, 0.0, 1.25], device='cuda') if scaled else None
                return lambda: _bwd(ops.linear_residual(x, w, b, res, sc))
            add(f'linear_residual C={C} scale={scaled}', make)

    for both in (True, False):
        def make(both=both):
            x, res = _t(2, 9, 20, 64, dt=BF, grad=True), _t(2, 9, 20, 64, dt=BF, grad=True)
            w, b = _t(64, 64, 1, 1, grad=True), _t(64, grad=True)

            def run():
                d, s = ops.conv1x1_and_sum(x, w, b, res)
                _bwd([d, s] if both else [s])
            return run
        add(f'conv1x1_and_sum both={both}', make)

    for C, both in ((32, True), (32, False), (64, True)):
        def make(C=C, both=both):
            y, skip = _t(2, 6, 10, C, dt=BF, grad=True), _t(2, 12, 20, C, dt=BF, grad=True)
            w, b = _t(C, C, 1, 1, grad=True), _t(C, grad=True)

            def run():
                d, s = ops.up_skip_conv(y, skip, w, b)
                _bwd([d, s] if both else [s])
            return run
        add(f'up_skip_conv C={C} both={both}', make)

    for Ci, Co, KH, KW, pre, post, has_bn, tok in INFER:
        def make(Ci=Ci, Co=Co, KH=KH, KW=KW, pre=pre, post=post, has_bn=has_bn, tok=tok):
            x = _t(2, 19 * 70, Ci, dt=BF) if tok else _t(2, 19, 70, Ci, dt=BF)
            w, b = (_t(Co, Ci) if tok else _t(Co, Ci, KH, KW)), _t(Co)
            bn = _bn(Co) if has_bn else None

            def run():
                with torch.no_grad():
                    ops.conv_bn_act(x, w, b, 1, (KH // 2, KW // 2), bn, pre, post)
            return run
        add(f'conv_bn_act {Ci}->{Co} {KH}x{KW} pre={pre} post={post} bn={has_bn} tokens={tok}', make)
    return out


def record_cases(case_list=None):
    """-> (cases {name: calls}, symbols): every case once as it stands and once inside begin_step / end_step (the pre-zeroed pool; the second pooled step
    over the same weights, the one recorded, takes its packs out of the step's single pack launch).  case_list: another set of [(name, make)] than cases()"""
    from tcct_amd import ops
    res, symbols = {}, {}
    torch.manual_seed(7)
    for name, make in (cases() if case_list is None else case_list):
        run = make()
        rec = _record(run)
        res[name] = rec.calls
        symbols.update(rec.symbols)

        def pooled():
            ops.begin_step('cuda')
            try:
                run()
            finally:
                ops.end_step()
        pooled()
        rec = _record(pooled)
        res[name + ' | pooled'] = rec.calls
        symbols.update(rec.symbols)
        del run, pooled
    return res, symbols


SAME = 'same calls as outside begin_step / end_step'


def encode(calls, symbols):
    last, out = {}, []
    for sym, vals in calls:
        vals = [v[0] + json.dumps(v[1], separators=(',', ':')) if isinstance(v, list) else v for v in vals]
        prev, last[sym] = last.get(sym), vals
        if prev is None:
            out.append([symbols.index(sym), vals])
        else:
            out.append([symbols.index(sym)] + [e for i, (a, b) in enumerate(zip(prev, vals)) if a != b
                                               for e in (i, f'{b - a:+d}' if type(a) is int and type(b) is int else b)])
    return _fold(out)


def _fold(ent):
    """consecutive repetitions of a block of entries -> ["*", n, block]; at each position the (period, count) that saves most"""
    out, i = [], 0
    while i < len(ent):
        saved, p, n = 0, 1, 1
        for q in range(1, min(64, (len(ent) - i) // 2) + 1):
            m = 1
            while ent[i + m * q:i + (m + 1) * q] == ent[i:i + q]:
                m += 1
            if (m - 1) * q > saved:
                saved, p, n = (m - 1) * q, q, m
        out.append(['*', n, ent[i:i + p]] if n > 1 else ent[i])
        i += n * p
    return out


def decode(enc, symbols):
    last, out = {}, []
    for e in [x for e in enc for x in (e[1] * e[2] if e[0] == '*' else [e])]:
        sym = symbols[e[0]]
        if len(e) == 2 and isinstance(e[1], list):
            vals = list(e[1])
        else:
            changed = dict(zip(e[1::2], e[2::2]))
            vals = [changed.get(i, v) for i, v in enumerate(last[sym])]
            vals = [a + int(v) if isinstance(v, str) and v[0] in '+-' else v for a, v in zip(last[sym], vals)]
        last[sym] = vals
        out.append([sym, [[v[:v.index('[')], json.loads(v[v.index('['):])] if isinstance(v, str) and v.endswith(']') else v for v in vals]])
    return out


def decode_cases(golden):
    """the `cases` of a loaded fixture -> {name: calls} in the form Recorder keeps them"""
    symbols, out = sorted(golden['symbols']), {}
    for name, enc in golden['cases'].items():
        out[name] = out[name[:-len(' | pooled')]] if enc == SAME else decode(enc, symbols)
    return out


def canonical(calls):
    return json.dumps(calls, separators=(',', ':'))


def digest(calls):
    per = {}
    for sym, _ in calls:
        per[sym] = per.get(sym, 0) + 1
    return {'calls': len(calls), 'per_symbol': dict(sorted(per.items())), 'sha256': hashlib.sha256(canonical(calls).encode()).hexdigest()}


def record_steps(arms=None):
    """-> {name: calls}: one KiteSeg.train_step (after one warm-up step) and one predict of stc_tt at 2 x 64 x 64 with --los=di+reg+fpl, bf16 and fp32.
    arms: [(name, command-line arguments beside the fixed ones)] instead -- bf16 train steps only, named `name`"""
    from tcct_amd.kite.main import parse_args
    from tcct_amd.data import SynthOCT
    from tcct_amd import nets
    from tcct_amd.kite.loop_seg import KiteSeg
    import tempfile
    res = {}
    for name, argv in arms or [(None, ['--los=di+reg+fpl', f'--dtype={dtype}']) for dtype in ('bf16', 'fp32')]:
        torch.manual_seed(2023)
        torch.cuda.manual_seed_all(2023)
        with tempfile.TemporaryDirectory() as root:
            args = parse_args(argv + ['--bs=2', '--db=synth', '--pl=false', f'--root={root}'])
            dtype = args.dtype
            ds = SynthOCT(height=64, width=64, device='cuda')
            net = nets.stc_tt(ds.out_channels, compute_dtype=BF if dtype == 'bf16' else F32, **(dict(legacy_heads=True) if args.legacy_heads else {}),
                              **(dict(att=args.att) if args.att != 'pool' else {}))
            net = nets.RegNet(net, con=args.type_udh, out_channels=ds.out_channels)
            k = KiteSeg(model=net, dataset=ds, root=args.root, args=args)
            k.model.train()
            img, lab, _, _ = ds.parse(ds.make_batch(2, seed=2023))
            img, lab = img.contiguous(), lab.contiguous()
            k.train_step(img, lab)
            torch.cuda.synchronize()
            res[name or f'train_step {dtype}'] = _record(lambda: k.train_step(img, lab)).calls
            if name is None:
                k.model.eval()
                res[f'predict {dtype}'] = _record(lambda: k.predict(img)).calls
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=FIXTURE)
    p.add_argument('--steps-full', metavar='DIR', default=None, help='also write the full call sequence of every whole step as DIR/<name>.json (one call per line)')
    a = p.parse_args()
    write_fixture(a.out, *record_cases(), record_steps(), a.steps_full)


def write_fixture(out, case_calls, symbols, steps, steps_full=None):
    if steps_full:
        os.makedirs(steps_full, exist_ok=True)
        for name, calls in steps.items():
            with open(os.path.join(steps_full, name.replace(' ', '_') + '.json'), 'w') as f:
                f.write('\n'.join(canonical(c) for c in calls) + '\n')
    with open(out, 'w') as f:
        f.write('{"symbols": {\n' + ',\n'.join(f'{json.dumps(s)}: {json.dumps(n)}' for s, n in sorted(symbols.items())) + '},\n"cases": {\n')
        names = sorted(symbols)
        enc = {n: SAME if n.endswith(' | pooled') and c == case_calls[n[:-len(' | pooled')]] else encode(c, names) for n, c in case_calls.items()}
        f.write(',\n'.join(f'{json.dumps(n)}: {canonical(e)}' for n, e in enc.items()) + '},\n"steps": {\n')
        f.write(',\n'.join(f'{json.dumps(n)}: {json.dumps(digest(c))}' for n, c in steps.items()) + '}}\n')
    print(f'{out}: {len(case_calls)} cases, {sum(len(c) for c in case_calls.values())} calls; steps: '
          + ', '.join(f'{n} {len(c)}' for n, c in steps.items()))


if __name__ == '__main__':
    main()
