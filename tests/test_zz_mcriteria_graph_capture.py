"""GPU: a captured training step with a criterion of get_mloss (sorts late, beside the other capture test of a non-default criterion): the nodes make no host
synchronisation and read their class weights from a persistent device buffer, so they replay from a hipGraph."""
import pytest
import torch

from test_mcriteria_gpu import make_mkite

pytestmark = pytest.mark.gpu


def test_graphed_step_with_weighted_cross_entropy_matches_eager(tmp_path):
    """one --graph=true step (tcct_amd.graph.GraphedTrainStep) with the weighted cross-entropy criterion against the eager step from the same state (structure and
    bounds of test_graphed_step_with_a_non_dice_criterion_matches_eager)"""
    from conftest import run_in_fresh_process
    if run_in_fresh_process(__file__, 'test_graphed_step_with_weighted_cross_entropy_matches_eager'):
        return
    import tcct_oracle as O
    from tcct_amd.graph import GraphedTrainStep
    k = make_mkite(tmp_path, torch.bfloat16, 'ce', [1.0, 1.0, 2.0, 2.0, 1.0], lr=1e-3)
    assert k.criterion.kind == 'ce' and k.criterion.class_w.is_cuda
    gstep = GraphedTrainStep(k, warmup=2)
    batches = [tuple(t.cuda() for t in O.synth_batch(2, 64, 96, seed=20 + i)) for i in range(4)]
    for i in range(3):                      # 2 eager warm-up steps on the capture stream, then capture + first replay
        gstep(*batches[i])
    assert gstep.graph is not None
    f = k.optimG._flat
    s0 = (f['p'].clone(), f['m'].clone(), f['v'].clone(), k.optimG.device_state.clone(), k.optimG._step, {n: b.clone() for n, b in k.model.named_buffers()})
    lg = gstep(*batches[3]).item()
    pg = f['p'].clone()
    f['p'].copy_(s0[0]); f['m'].copy_(s0[1]); f['v'].copy_(s0[2]); k.optimG.device_state.copy_(s0[3]); k.optimG._step = s0[4]
    for n, b in k.model.named_buffers():
        b.copy_(s0[5][n])
    k.optimG._lr_pushed = None
    k.optimG.sync_lr()
    le = k.train_step(*batches[3]).item()
    pe = f['p'].clone()
    upd, dif = (pe - s0[0]).abs().max().item(), (pe - pg).abs().max().item()
    print(f'    loss graph {lg:.6f} eager {le:.6f}; max |update| {upd:.3e}, max |graph - eager| {dif:.3e}')
    assert abs(lg - le) < 1e-4 * abs(le) and dif < 2e-2 * upd and upd > 0, (lg, le, upd, dif)
