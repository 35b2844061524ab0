"""f1, training-mode Conv blocks, host side: the trainer's parameter groups of train.ParamGroups / ConvBN and the algebra of ConvBN.fold()
(plain torch) against nn.BatchNorm2d in .eval() -- CPU tensors, no device needed."""
import pytest
import torch
import torch.nn as nn


def _block(c1, c2, k, s, seed):
    import oriented_object_detection_amd.train as TR
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(c2, c1, k, k, generator=g) * 0.2
    gamma, beta = torch.rand(c2, generator=g) + 0.5, torch.randn(c2, generator=g) * 0.2
    rm, rv = torch.randn(c2, generator=g) * 0.3, torch.rand(c2, generator=g) + 0.2
    grp = TR.ParamGroups("SGD", lr=0.01, weight_decay=5e-4)
    blk = TR.ConvBN(grp, w, gamma, beta, s=s, running_mean=rm, running_var=rv)
    grp.build()
    return grp, blk, (w, gamma, beta, rm, rv)


@pytest.mark.parametrize("c1,c2,k,s", [(16, 24, 1, 1), (8, 16, 3, 1), (16, 16, 3, 2)])
def test_convbn_fold_matches_batchnorm_eval(c1, c2, k, s):
    """BN(eval) is a per-channel affine map y -> f y + b and the conv is linear in its weights, so bn_eval(conv(x, w)) = conv(x, wf) + bf holds
    exactly when wf[co] = f[co] w[co] and bf = b.  Both come from nn.BatchNorm2d.eval() itself: applied to the weights laid out as a batch of
    c1*k*k samples of c2 channels it gives f w + b, applied to zeros it gives b."""
    grp, blk, (w, gamma, beta, rm, rv) = _block(c1, c2, k, s, c1 + c2 + k + s)
    bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    bn.eval()
    with torch.no_grad():
        b_ref = bn(torch.zeros(1, c2, 1, 1)).reshape(c2)
        wt = w.permute(1, 2, 3, 0).reshape(-1, c2, 1, 1)  # [c1*k*k samples][c2 channels]
        wf_ref = (bn(wt).reshape(c1, k, k, c2) - b_ref).permute(3, 0, 1, 2)
    wf, bf = blk.fold()
    assert wf.shape == w.shape and bf.shape == (c2,)
    assert float((wf - wf_ref).abs().max()) <= 1e-5 * float(wf_ref.abs().max())
    assert float((bf - b_ref).abs().max()) <= 1e-6 * float(b_ref.abs().max())


def test_convbn_parameters_live_in_the_trainer_groups():
    """conv weight -> group 0 (decay), gamma -> group 1, beta -> group 2 (no decay): views of the FlatOptimizers' buffers; running statistics
    are buffers of the block, not parameters."""
    grp, blk, (w, gamma, beta, rm, rv) = _block(8, 16, 3, 2, 1)
    assert [o.n for o in grp.opts] == [w.numel(), 16, 16]
    assert [o.weight_decay for o in grp.opts] == [5e-4, 0.0, 0.0]
    assert blk.w.data_ptr() == grp.opts[0].param.data_ptr() and blk.dw.data_ptr() == grp.opts[0].grad.data_ptr()
    assert blk.gamma.data_ptr() == grp.opts[1].param.data_ptr() and blk.dbeta.data_ptr() == grp.opts[2].grad.data_ptr()
    assert torch.equal(blk.w, w) and torch.equal(blk.gamma, gamma) and torch.equal(blk.beta, beta)
    assert torch.equal(blk.running_mean, rm) and torch.equal(blk.running_var, rv)
    assert sum(o.n for o in grp.opts) == w.numel() + 32  # running statistics are not in any group


def test_convbn_rejects_unbuilt_shapes():
    import oriented_object_detection_amd.train as TR
    grp = TR.ParamGroups()
    with pytest.raises(ValueError):
        TR.ConvBN(grp, torch.zeros(8, 8, 1, 1), s=2)  # stride 2 exists for 3x3 only
    with pytest.raises(ValueError):
        TR.ConvBN(grp, torch.zeros(8, 8, 5, 5))
