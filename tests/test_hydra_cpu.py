"""att='hydra': the reference's HydraAttention token mixer (nets/tcct.py:343-403, commented out in MHCABlock tcct.py:435-441) -- everything that
needs no GPU: the constructor surface, the CLI, the C-ABI declarations, and a plain-torch restatement of the mixer pinned to fixtures recorded
from the real reference classes (tools/make_golden_hydra.py).  The restatement (`hydra_att_mix` / `hydra_att`) is the rounding model of
tests/test_hydra_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))

CASES = ('hy64', 'hy96', 'hy128', 'hy160')
FORMULA_ONLY = ('qkv.weight', 'proj.weight')        # not stored for the wide cases: formula_tensor(f'{tag}.{key}') exactly (asserted by the generator)


def _same(t):
    return t


def hydra_att_mix(x, qkv_w, qkv_b, crpe_wb, size, heads, qk_scale=None, store=_same, wcast=_same):
    """HydraAttention.forward up to (not including) the output projection, written from the formulas:
        qn = q / |q|, kn = k / |k|  (norm over the Ch channels of one head of one token, no epsilon)
        kv[b,h,c] = sum_n kn * v
        mix = scale * qn * kv + q * crpe_conv(v),  scale = Ch ** -0.5
    x [B,N,C] tokens, size = (H, W); crpe_wb = [(weight [Cg,1,k,k], bias [Cg]), ...] in conv_list order (windows 3/5/7 over 2+3+3 of 8 heads).
    store / wcast: identity = fp32 arithmetic; the bf16 tests pass a differentiable round-to-bf16, applied to every tensor the HIP path keeps in
    memory (qkv, the crpe convolution, the output) and to the GEMM weights -- the same hooks as tcct_oracle.factor_att_mix."""
    B, N, C = x.shape[0], x.shape[1], qkv_w.shape[0] // 3
    H, W = size
    Ch = C // heads
    scale = qk_scale or Ch ** -0.5
    qkv = store(F.linear(x, wcast(qkv_w), qkv_b)).reshape(B, N, 3, heads, Ch)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]                  # [B,N,h,Ch]
    qn = q / q.pow(2).sum(-1, keepdim=True).sqrt()
    kn = k / k.pow(2).sum(-1, keepdim=True).sqrt()
    kv = (kn * v).sum(1, keepdim=True)                                   # [B,1,h,Ch]
    v_img = v.reshape(B, H, W, C).permute(0, 3, 1, 2)                    # channel = head*Ch + ch
    parts, off = [], 0
    for w, b in crpe_wb:
        cg, kk = w.shape[0], w.shape[2]
        parts.append(F.conv2d(v_img[:, off:off + cg], w, b, 1, kk // 2, 1, cg))
        off += cg
    cv = store(torch.cat(parts, 1).permute(0, 2, 3, 1)).reshape(B, N, heads, Ch)
    return store((scale * qn * kv + q * cv).reshape(B, N, C))


def hydra_att(x, qkv_w, qkv_b, proj_w, proj_b, crpe_wb, size, heads, qk_scale=None, store=_same, wcast=_same):
    return store(F.linear(hydra_att_mix(x, qkv_w, qkv_b, crpe_wb, size, heads, qk_scale, store, wcast), wcast(proj_w), proj_b))


def load_case(tag):
    """fixture of one case as torch tensors, the formula-only GEMM weights of the wide cases rebuilt"""
    import tcct_oracle as O
    fname = 'hydraatt.npz' if tag in ('hy64', 'hy96') else 'hydraatt_wide.npz'
    fx = {k[len(tag) + 1:]: torch.tensor(v) for k, v in np.load(os.path.join(HERE, 'golden', fname)).items() if k.startswith(tag + '.')}
    for k in FORMULA_ONLY:
        if 'p.' + k not in fx:
            fx['p.' + k] = O.formula_tensor(f'{tag}.{k}', tuple(fx['g.' + k].shape))
    return fx


def run_restatement(fx, store=_same, wcast=_same, cast=_same):
    """-> (y, dx, {parameter name: gradient}) of the restatement on the fixture's inputs"""
    H, W = (int(v) for v in fx['size'])
    x = cast(fx['x']).clone().requires_grad_(True)
    ps = {k[2:]: v.clone().requires_grad_(True) for k, v in fx.items() if k.startswith('p.')}
    wb = [(ps[f'crpe.conv_list.{i}.weight'], ps[f'crpe.conv_list.{i}.bias']) for i in range(3)]
    y = hydra_att(x, ps['qkv.weight'], ps['qkv.bias'], ps['proj.weight'], ps['proj.bias'], wb, (H, W), int(fx['heads']), store=store, wcast=wcast)
    y.backward(cast(fx['gout']))
    return y.detach(), x.grad, {k: p.grad for k, p in ps.items()}


@pytest.mark.parametrize('tag', CASES)
def test_restatement_reproduces_reference_fixture(tag):
    """the real reference classes' forward / backward (HydraAttention + ConvRelPosEnc) against the formulas, at the tolerances
    oracle/make_golden_factoratt.py uses for its own restatement"""
    fx = load_case(tag)
    assert fx['x'].shape[-1] // int(fx['heads']) == {'hy64': 8, 'hy96': 12, 'hy128': 16, 'hy160': 20}[tag]
    y, dx, g = run_restatement(fx)
    assert torch.allclose(y, fx['y'], rtol=1e-5, atol=1e-6), float((y - fx['y']).abs().max())
    assert torch.allclose(dx, fx['dx'], rtol=1e-5, atol=1e-6), float((dx - fx['dx']).abs().max())
    assert set(g) == {k[2:] for k in fx if k.startswith('g.')}
    for k, gk in g.items():
        ref = fx['g.' + k]
        assert torch.allclose(gk, ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max())), k


def test_hydra_option_mirrors_the_factor_key_set():
    """stc_tt(att='hydra') registers exactly what att='factor' registers (HydraAttention has the constructor of FactorAtt_ConvRelPosEnc,
    reference tcct.py:346-367): same keys, same shapes, the att.crpe.* keys aliasing the shared ConvRelPosEnc; 8 heads"""
    from tcct_amd.nets import stc_tt
    from tcct_amd.nets.tcct import HydraAttention
    fa, hy = stc_tt(5, att='factor').state_dict(), stc_tt(5, att='hydra').state_dict()
    assert list(fa) == list(hy)
    assert all(fa[k].shape == hy[k].shape for k in fa)
    net = stc_tt(5, att='hydra')
    for s in range(4):
        blk = f'base_vit.mhca_stages.{s}.mhca_blks.0'
        assert hy[f'{blk}.MHCA_layers.0.att.crpe.conv_list.0.weight'].data_ptr() == hy[f'{blk}.crpe.conv_list.0.weight'].data_ptr()
        enc = net.base_vit.mhca_stages[s].mhca_blks[0]
        att = enc.MHCA_layers[0].att
        assert isinstance(att, HydraAttention) and att.num_heads == 8 and att.crpe is enc.crpe
        assert att.scale == (net.base_vit.embed_dims[s] // 8) ** -0.5
    with pytest.raises(ValueError, match='hydra'):
        stc_tt(5, att='bogus')


def test_whole_network_fixture_has_our_key_set():
    """the key / shape list recorded from the reference network with HydraAttention assigned to its blocks == RegNet(stc_tt(att='hydra'))"""
    from tcct_amd.nets import stc_tt, RegNet
    fx = np.load(os.path.join(HERE, 'golden', 'hydra_net_2x64x128.npz'))
    ref = {str(k): tuple(int(d) for d in str(s).split(',') if d) for k, s in zip(fx['key_names'], fx['key_shapes'])}
    ours = {k: tuple(v.shape) for k, v in RegNet(stc_tt(5, att='hydra'), con='cos', out_channels=5).state_dict().items()}
    assert ours == ref


@pytest.mark.parametrize('tag', CASES)
def test_module_accepts_the_reference_parameter_names(tag):
    from tcct_amd.nets.tcct import HydraAttention, ConvRelPosEnc
    fx = load_case(tag)
    heads, dim = int(fx['heads']), fx['x'].shape[-1]
    att = HydraAttention(dim, num_heads=heads, qkv_bias=True, shared_crpe=ConvRelPosEnc(Ch=dim // heads, h=heads, window={3: 2, 5: 3, 7: 3}))
    res = att.load_state_dict({k[2:]: v for k, v in fx.items() if k.startswith('p.')}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert hasattr(att, 'mix') and att.crpe.conv_list[2].weight.shape[-1] == 7


def test_cli_offers_hydra():
    from tcct_amd.kite.main import parse_args, main
    assert parse_args(['--att=hydra']).att == 'hydra' and parse_args(['--att=factor']).att == 'factor' and parse_args([]).att == 'pool'
    with pytest.raises(SystemExit):
        parse_args(['--att=bogus'])


def test_header_declares_the_hydra_entries():
    from tcct_amd._lib import parse_header
    protos = parse_header()
    for name in ('tcct_hydra_kv', 'tcct_hydra_dkv', 'tcct_hydra_apply_fwd', 'tcct_hydra_apply_bwd'):
        res, sig = protos[name]
        assert sig[-1][1] == 'stream' and any(nm == 'dtype' for _, nm in sig) and any(nm == 'heads' for _, nm in sig), name
    assert [nm for _, nm in protos['tcct_hydra_kv_workspace_bytes'][1]] == ['B', 'N', 'C']
    assert any(nm == 'workspace' for _, nm in protos['tcct_hydra_kv'][1]) and any(nm == 'workspace' for _, nm in protos['tcct_hydra_dkv'][1])
