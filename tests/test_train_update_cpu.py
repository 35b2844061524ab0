"""The host side of the trainer update (train.Schedule, ModelEMA's decay, ParamGroups' buffer of running statistics, the `_Step.update` hook) --
no GPU: the schedule against an np.interp restatement written here, the decay curve against its closed form, the rebinding of
`blk.running_mean` / `running_var` on CPU tensors."""
import math

import numpy as np
import pytest
import torch

import train_update_ref as UR


def _tr():
    import oriented_object_detection_amd  # noqa: F401
    import oriented_object_detection_amd.train as TR
    return TR


def schedule_ref(ni, epoch, *, epochs, nb, lr0, lrf, momentum, cos_lr, warmup_epochs=3.0, warmup_momentum=0.8, warmup_bias_lr=0.1, batch=16, nbs=64):
    """Ultralytics' warm-up and lr rules (8.3.x, recalled) written out with np.interp, sharing no code with train.Schedule -> (lr_w, lr_norm, lr_bias,
    momentum, accumulate).  The cosine lf is the trainer's own expression."""
    nw = max(round(warmup_epochs * nb), 100)
    if cos_lr:
        lf = ((1 - math.cos(epoch * math.pi / epochs)) / 2) * (lrf - 1) + 1
    else:
        lf = max(1 - epoch / epochs, 0) * (1.0 - lrf) + lrf
    lrs, mom, acc = [lr0 * lf] * 3, momentum, max(1, round(nbs / batch))
    if ni <= nw:
        xi = [0, nw]
        acc = max(1, int(np.interp(ni, xi, [1, nbs / batch]).round()))
        lrs = [float(np.interp(ni, xi, [warmup_bias_lr if j == 2 else 0.0, lr0 * lf])) for j in range(3)]
        mom = float(np.interp(ni, xi, [warmup_momentum, momentum]))
    return lrs[0], lrs[1], lrs[2], mom, acc


# nb = 10: 3 warm-up epochs are 30 iterations, so the floor of 100 applies; nb = 200: nw = 600
@pytest.mark.parametrize("nb", [10, 200])
@pytest.mark.parametrize("cos_lr", [False, True])
def test_schedule_against_interp_restatement(nb, cos_lr):
    TR = _tr()
    kw = dict(epochs=50, nb=nb, lr0=0.003, lrf=0.05, momentum=0.937, cos_lr=cos_lr)
    s = TR.Schedule(**kw)
    nw = s.nw
    assert nw == (100 if nb == 10 else 600)
    last = 50 * nb - 1
    for ni in (0, 1, nw - 1, nw, nw + 1, last):
        epoch = ni // nb
        got = s.at(ni, epoch)
        ref = schedule_ref(ni, epoch, **kw)
        assert got["accumulate"] == ref[4] and isinstance(got["accumulate"], int)
        for g, r in zip((*got["lr"], got["momentum"]), ref[:4]):
            assert g == pytest.approx(r, rel=4 * 2.0 ** -52, abs=0)  # (the cosine lf is written in another, end-exact, form)
        if not cos_lr:
            assert (*got["lr"], got["momentum"]) == ref[:4]
    first = s.at(0, 0)
    assert first["lr"] == (0.0, 0.0, 0.1) and first["momentum"] == 0.8 and first["accumulate"] == 1
    assert s.at(nw, nw // nb)["accumulate"] == 4 and s.at(last, last // nb)["accumulate"] == 4  # batch 16, nbs 64: 1 -> 4
    assert s.at(nw + 1, (nw + 1) // nb)["momentum"] == 0.937


@pytest.mark.parametrize("cos_lr", [False, True])
def test_bias_group_ramps_down_while_the_others_ramp_up(cos_lr):
    TR = _tr()
    s = TR.Schedule(epochs=50, nb=10, lr0=0.003, lrf=0.05, cos_lr=cos_lr)
    seq = [s.at(ni, 2) for ni in range(0, s.nw + 1)]  # (within one epoch: the ramp's target lr0 lf(epoch) itself steps down at every epoch)
    w, nrm, b = ([q["lr"][j] for q in seq] for j in range(3))
    assert w == nrm
    assert all(x < y for x, y in zip(w, w[1:])) and w[0] == 0.0
    assert all(x > y for x, y in zip(b, b[1:])) and b[0] == 0.1
    end = 0.003 * s.lf(2)
    assert b[-1] == w[-1] == end and 0.003 * 0.05 < end < 0.003
    mom = [q["momentum"] for q in seq]
    assert all(x < y for x, y in zip(mom, mom[1:])) and (mom[0], mom[-1]) == (0.8, 0.937)


@pytest.mark.parametrize("cos_lr", [False, True])
def test_lrf_end_points_are_exact(cos_lr):
    TR = _tr()
    s = TR.Schedule(epochs=50, nb=200, lr0=0.003, lrf=0.05, cos_lr=cos_lr)
    assert s.lf(0) == 1.0 and s.lf(50) == 0.05
    assert s.at(10 ** 6, 0)["lr"] == (0.003,) * 3            # past the warm-up, first epoch's factor: exactly lr0
    assert s.at(10 ** 6, 50)["lr"] == (0.003 * 0.05,) * 3    # lr0 lrf
    mid = s.lf(25)
    assert mid == pytest.approx(0.525, rel=1e-15)            # both forms meet half-way: (1 + lrf) / 2


def test_accumulate_follows_batch():
    TR = _tr()
    assert TR.Schedule(10, 10, 0.01, batch=64).at(10 ** 6, 0)["accumulate"] == 1
    assert TR.Schedule(10, 10, 0.01, batch=32).at(10 ** 6, 0)["accumulate"] == 2
    s = TR.Schedule(10, 10, 0.01, batch=16)
    assert [s.at(ni, 0)["accumulate"] for ni in (0, 16, 17, 50, 83, 84, 100)] == [1, 1, 2, 2, 3, 4, 4]
    with pytest.raises(ValueError):
        TR.Schedule(0, 10, 0.01)


def test_ema_decay_curve():
    TR = _tr()
    g = TR.ParamGroups()  # (the decay needs no device: a built ParamGroups of CPU tensors)
    blk = TR.ConvBN(g, torch.randn(8, 8, 1, 1))
    g.build()
    ema = TR.ModelEMA(g, decay=0.9999, tau=2000)
    for updates, ref in ((1, 0.9999 * (1 - math.exp(-1 / 2000))), (2000, 0.9999 * (1 - math.exp(-1.0))), (10 ** 6, 0.9999)):
        assert ema.decay_at(updates) == pytest.approx(ref, rel=1e-15)
        assert ema.decay_at(updates) == UR.ema_decay(updates)
    assert ema.decay_at(1) == pytest.approx(4.998e-4, rel=1e-3) and ema.decay_at(10 ** 6) == 0.9999
    assert [tuple(t.shape) for t in ema.ema] == [(64,), (8,), (8,), (16,)]
    assert ema.ema[3].data_ptr() != g.buffers.data_ptr() and torch.equal(ema.ema[3], g.buffers) and blk.running_var.data_ptr() != ema.ema[3].data_ptr()
    with pytest.raises(RuntimeError):
        TR.ModelEMA(TR.ParamGroups())


def test_running_statistics_live_in_the_groups_buffer():
    TR = _tr()
    g = TR.ParamGroups()
    rm0 = torch.arange(16, dtype=torch.float32)
    a = TR.ConvBN(g, torch.randn(16, 8, 3, 3), running_mean=rm0)
    b = TR.DWConvBN(g, torch.randn(8, 1, 3, 3))
    c = TR.StemConvBN(g, torch.randn(24, 3, 3, 3))
    assert len(g.buffer_items) == 6
    for blk, n0 in ((a, 0), (b, 2), (c, 4)):  # exactly two each, mean then var
        assert [(o is blk, at) for o, at in g.buffer_items[n0:n0 + 2]] == [(True, "running_mean"), (True, "running_var")]
    before = torch.full((8,), 7.5)
    b.running_var.copy_(before)               # a value copied in BEFORE build() ...
    g.build()
    assert g.buffers.numel() == 2 * (16 + 8 + 24) and g.buffers.dtype == torch.float32
    assert torch.equal(b.running_var, before) and torch.equal(a.running_mean, rm0)      # ... survives it
    off = 0
    for blk in (a, b, c):
        for t in (blk.running_mean, blk.running_var):
            assert t.data_ptr() == g.buffers.data_ptr() + 4 * off and t.shape == (blk.c2,)
            off += blk.c2
    assert torch.equal(g.buffers[32:40], torch.zeros(8)) and torch.equal(g.buffers[40:48], before) and torch.equal(g.buffers[72:], torch.ones(24))
    c.running_mean.copy_(torch.full((24,), -2.0))  # a copy_ AFTER build() lands in the flat buffer
    assert torch.equal(g.buffers[48:72], torch.full((24,), -2.0))
    w, bias = c.fold()                        # fold() reads the views
    assert torch.allclose(bias, 2.0 / torch.sqrt(torch.tensor(1.0 + 1e-3)) * torch.ones(24))
    with pytest.raises(RuntimeError):
        g.add_buffer(a.running_mean, a, "running_mean")
    assert sum(o.n for o in g.opts) == (16 * 72 + 8 * 9 + 24 * 27) + 2 * (16 + 8 + 24)  # the statistics are in no parameter group


def test_groups_without_buffers_build_an_empty_one():
    TR = _tr()
    g = TR.ParamGroups()
    TR.HeadOut(g, torch.randn(3, 8, 1, 1), torch.zeros(3))
    g.build()
    assert g.buffers.numel() == 0


def test_step_hands_over_to_the_update_when_one_is_set():
    TR = _tr()
    calls = []

    class Groups:
        def flat_grads(self):
            return []

        def step(self):
            calls.append("groups.step")

    class M(TR._Step):
        groups = Groups()

        def forward_backward(self, x, scale=1):
            calls.append(("fb", x, scale))
            return x * scale

    m = M()
    assert m.step(3, scale=2) == 6 and calls == [("fb", 3, 2), "groups.step"]
    with pytest.raises(TypeError):
        m.step(3, ni=0, epoch=0)
    del calls[:]
    m.update = lambda ni, epoch, group=None: calls.append(("update", ni, epoch, group)) or "clip"
    assert m.step(3, scale=2, ni=7, epoch=1, group="pg") == 6
    assert calls == [("fb", 3, 2), ("update", 7, 1, "pg")] and m.last_clip == "clip"
    with pytest.raises(TypeError):
        m.step(3)
