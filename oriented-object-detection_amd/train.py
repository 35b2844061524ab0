"""Training-step slices behind `model.train(...)` (Train_OBB.py:796-841) that sit BETWEEN the loss / backward
kernels (loss.py, ops.conv_dgrad_bf16 / conv_wgrad_bf16, ops.rotated_tal_assign) and the next forward:

  * `optimizer_config` / `param_group_of`: Ultralytics' `BaseTrainer.build_optimizer` rules (ultralytics==8.3.x, recalled -- the package
    is not installed here, so this restatement is UNPINNED; the numerics below are pinned against torch.optim itself): optimizer "auto"
    = SGD(lr 0.01, momentum 0.9, nesterov) above 10 000 iterations, else AdamW(lr = round(0.002 * 5 / (4 + nc), 6), betas (0.9, 0.999));
    three groups: biases (no decay), norm weights (no decay), other weights (decay = weight_decay * batch * accumulate / nbs);
  * `FlatOptimizer`: a parameter group as ONE flat fp32 device buffer (parameters, gradients, state) updated by one HIP launch
    (csrc/optim.hip) -- the arithmetic of torch.optim.SGD / AdamW, checked against them step by step;
  * `allreduce_gradients`: the DDP gradient average of `device="0,1"` (Train_OBB.py: DEVICE) as bucketed all-reduces over
    torch.distributed (backend "nccl" = RCCL over xGMI on the GPU box; gloo in the CPU test): the flat gradient buffers are already
    contiguous, so a bucket is a view, not a copy; buckets of `bucket_mb` keep a ring all-reduce per-link bandwidth-bound rather than
    latency-bound (7 xGMI links x ~153 GB/s per GPU: a 25 MB bucket is ~0.1 ms of wire time per hop);
  * `ParamGroups` / `ConvBN` / `DetectBoxBranchStep`: the trainer's three groups as FlatOptimizers, the Ultralytics `Conv` block in
    training mode (batch-statistics BatchNorm + SiLU, stride 1 or 2) and the head's box branch built from it, BatchNorm unfolded;
    `wgrad_route` names the block class a layer's weight gradient runs in (csrc/convgrad.hip's k_conv_wgrad: 64 x 64 blocks of dW, or blocks at
    their live width for the other multiples of 8), so ConvBN trains at every dense conv shape of YOLO11 n / s with channels in multiples of 8;
    `train_kernel_of` names the kernel family of ANY conv of the model ("dense" / "depthwise" / "stem" / "head_out");
  * `_BNBlock`: what the three BatchNorm blocks `ConvBN`, `DWConvBN` and `StemConvBN` are made of -- the registration of w / gamma / beta in groups
    0 / 1 / 2, the running statistics, the parameter and gradient views, `fold()`, and `forward` / `backward` as a conv half around
    ops.bn_fwd_bf16 / ops.bn_bwd_bf16 (`act`: with or without SiLU).  A subclass is its shape check and its two conv halves.  `_bn_block` builds
    one from a parameter tuple (w, gamma, beta[, running_mean, running_var]): every composite below takes its blocks as such tuples;
  * `_Composite`: every module that owns layers states `children()` = [(checkpoint-relative name, child)] once; `named_blocks()` (the leaves under
    dotted names), `fold()`, `Net.pack_layers` (the dense layers with their input maps, the stride known per top-level child) and `FoldPlan` are
    that one walk.  The leaves -- the three _BNBlocks and the two plain convs -- describe themselves: c1, c2, k, s, g, act, `fold()`, and `order`
    on a block held in another row order than the checkpoint's (Attention's qkv);
  * `StemConvBN` / `HeadOut`: the two layer kinds outside the multiples of 8 (csrc/narrowgrad.hip) -- model.0 on the 3- or 4-channel uint8 tile under
    ConvBN's contract, and the head's plain `Conv2d` 1x1 + bias outputs (nc class logits, 1 angle logit) with fp32 logits and a fused dx + dW + db
    backward; `BoxOut` is the box branch's 64-channel output under the same contract, on the dense kernels and with bf16 logits;
  * `SPPF` / `UpCat`: the joins between Conv blocks that are not convs -- SPPF's chained max pools, Upsample + Concat of the FPN, Concat of
    the PAN, and the gradient sum of a tensor with two consumers (csrc/routegrad.hip);
  * `DWConvBN` / `ClassBranchPair`: the depthwise 3x3 Conv block (csrc/dwgrad.hip: fused dx + dW backward; BatchNorm with or without SiLU) and
    one `DWConv 3x3 -> Conv 1x1` pair of the head's class branch built from it and ConvBN;
  * `Attention` / `PSABlock`: C2PSA's attention (csrc/attngrad.hip: the softmax core with its backward) and one PSA block of model 10 around it --
    qkv / proj / ffn as ConvBN (with `act=False` where the reference has none), pe as DWConvBN, the residual adds and the gradient sums at their
    fan-outs as ops.add_bf16;
  * `Bottleneck` / `C3k` / `C3k2` / `C2PSA`: the composite blocks of the trunk (models 2, 4, 6, 8, 10, 13, 16, 19, 22) assembled from the blocks above;
    `chunk` / `split` / `cat` and the gradient sums at the concat members are channel-window copies and adds (ops.chanwin_bf16, csrc/routegrad.hip);
  * `_Chain`: layers in a row, forward in order and backward reversed -- `ClassBranchPair` and the head's branches: `_DetectBoxBranch`
    (Detect.cv2[i]: two ConvBN, BoxOut), `DetectAngleBranch` (OBB.cv4[i]: the same ending in HeadOut; no loss of its own) and `_DetectClassBranch`
    (Detect.cv3[i]: two ClassBranchPairs, HeadOut);
  * `DetectBoxBranchStep` / `DetectClassBranchStep`: thin wrappers -- a box / class branch on parameter groups of its own under the DFL / BCE term
    (`_BranchStep`), with the one `step()` (`_Step`: forward_backward, DDP gradient average, optimiser step) that `DetectHead` uses too;
  * `pad_targets` / `OBBCriterion` / `DetectHead`: the criterion chain (csrc/criterion.hip) -- the host-side padding of the labels, v8OBBLoss from the
    head's logits to loss items and logit gradients without a host read (decode -> assigner -> fused loss), and the three levels of Detect / OBB
    (box, class and angle branches over one ParamGroups) trained under it;
  * `clip_grad_norm` / `Schedule` / `ModelEMA` / `TrainerUpdate`: the update half of the trainer's iteration (csrc/trainupd.hip) -- the global
    gradient-norm clip (max_norm 10) whose coefficient is produced and consumed on the device, the warm-up ramps of learning rate and momentum (the
    bias group ramping DOWN from warmup_bias_lr) followed by the linear or cosine `lrf` decay, gradient accumulation up to the nominal batch size,
    and the EMA of the weights AND the BatchNorm running statistics (`ParamGroups.buffers`), the model the trainer validates and saves.  One update
    is a fixed handful of launches over the flat group buffers whatever the number of layers (accumulate, sum of squares, coefficient, step of all
    three groups, EMA), none of which reads back to the host; `_Step.step(..., ni=, epoch=)` runs it when the module's `update` is set;
  * `FoldPlan` / `Validator`: the `val` pass behind every epoch of `model.train(...)` -- the flat buffers (live or the EMA's) folded into an "OBBW"
    weight blob by one launch (csrc/foldblob.hip), reloaded into an inference-engine slot of the validator's own (`model.YOLO.reload`), the pool's
    tiles run through it unaugmented, the detections matched to the targets at ten ProbIoU thresholds (csrc/valmatch.hip) and cumulated to
    mAP50 / mAP50-95 / fitness on the host (`metrics.ap_per_class`); `Net.validate` is the shorthand."""
import math
import struct

import torch

from . import ops


def optimizer_config(nc, iterations, name="auto", lr0=0.003, momentum=0.937, weight_decay=0.001, batch=16, nbs=64):
    """-> dict(name, lr, momentum, weight_decay, accumulate).  `name="auto"` ignores lr0 / momentum like the trainer does."""
    accumulate = max(round(nbs / batch), 1)
    wd = weight_decay * batch * accumulate / nbs
    if name == "auto":
        lr_fit = round(0.002 * 5 / (4 + nc), 6)
        name, lr0, momentum = ("SGD", 0.01, 0.9) if iterations > 10000 else ("AdamW", lr_fit, 0.9)
    if name not in ("SGD", "AdamW"):
        raise NotImplementedError(f"optimizer {name}: only the two that `auto` selects are built")
    return {"name": name, "lr": lr0, "momentum": momentum, "weight_decay": wd, "accumulate": accumulate}


def iterations_of(n_train_tiles, epochs, batch=16, nbs=64):
    """The trainer's iteration estimate that feeds `auto`: ceil(len(dataset) / max(batch, nbs)) * epochs."""
    return math.ceil(n_train_tiles / max(batch, nbs)) * epochs


def param_group_of(param_name, module_is_norm=False):
    """0 = weights with decay, 1 = norm weights (no decay), 2 = biases (no decay) -- the trainer's g[0] / g[1] / g[2]."""
    if "bias" in param_name:
        return 2
    if module_is_norm or "logit_scale" in param_name:
        return 1
    return 0


class FlatOptimizer:
    """One parameter group: `param` (flat fp32 device tensor, updated in place) with its optimiser state.  `views(shapes)` hands out the
    per-layer tensors as views of the flat buffer, so the layers' kernels write gradients straight into `grad`."""

    def __init__(self, n, device, name="SGD", lr=0.01, momentum=0.9, weight_decay=0.0, nesterov=True, betas=None, eps=1e-8):
        if name not in ("SGD", "AdamW"):
            raise NotImplementedError(name)
        self.name, self.lr, self.momentum, self.weight_decay, self.nesterov, self.eps = name, lr, momentum, weight_decay, nesterov, eps
        self.betas = betas or (momentum, 0.999)
        n4 = (n + 3) // 4 * 4
        self.n = n
        self.param = torch.zeros(n4, dtype=torch.float32, device=device)[:n]
        self.grad = torch.zeros(n4, dtype=torch.float32, device=device)[:n]
        self.state = [torch.zeros(n4, dtype=torch.float32, device=device)[:n] for _ in range(1 if name == "SGD" else 2)]
        self.steps = 0

    @staticmethod
    def views(flat, shapes):
        out, o = [], 0
        for s in shapes:
            k = int(math.prod(s))
            out.append(flat[o:o + k].view(*s))
            o += k
        if o != flat.numel():
            raise ValueError("views: the shapes do not cover the buffer")
        return out

    def step(self, lr=None):
        lr = self.lr if lr is None else lr
        self.steps += 1
        if self.name == "SGD":
            ops.sgd_step(self.param, self.grad, self.state[0], lr, self.momentum, self.weight_decay, self.nesterov, first_step=self.steps == 1)
        else:
            ops.adamw_step(self.param, self.grad, self.state[0], self.state[1], self.steps, lr, self.betas, self.eps, self.weight_decay)

    def zero_grad(self):
        self.grad.zero_()


def allreduce_gradients(flat_grads, group=None, bucket_mb=25.0, average=True):
    """Average the flat gradient buffers over the ranks of `group` in place: bucketed `all_reduce`s (views of the flat buffers, launched
    asynchronously, waited for at the end).  Returns the number of collectives issued.  World size 1 / no process group: nothing to do."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    world = dist.get_world_size(group)
    if world == 1:
        return 0
    per = max(1, int(bucket_mb * (1 << 20)) // 4)
    works = []
    for g in flat_grads:
        for o in range(0, g.numel(), per):
            works.append(dist.all_reduce(g[o:o + per], op=dist.ReduceOp.SUM, group=group, async_op=True))
    for w in works:
        w.wait()
    if average:
        for g in flat_grads:
            g.mul_(1.0 / world)
    return len(works)


class BoxBranchStep:
    """ONE assembled training step of the box branch of a head level (ultralytics Detect.cv2[i]: Conv 3x3 + SiLU, Conv 3x3 + SiLU, Conv2d 1x1
    -> 4 x 16 DFL logits per anchor; BatchNorm folded as in the OBBW blob) under the DFL term of the OBB loss -- what `loss.backward()` +
    `optimizer.step()` do to these three layers inside `model.train(...)` (Train_OBB.py:796-841; bf16 autocast over fp32 master weights):
        pack (device) -> conv -> SiLU -> conv -> SiLU -> conv -> DFL loss + gradient -> [wgrad, bias grad, dgrad, SiLU'] x 3 -> optimiser.
    Every arithmetic step is a kernel of libobbhip; the master weights live in two flat optimiser groups (weights with decay, biases
    without), the gradients are written straight into the groups' flat gradient buffers.  Activations and gradients between layers are bf16
    (one rounding per tensor), sums fp32."""

    def __init__(self, weights, biases, H, W, optimizer="SGD", lr=0.01, momentum=0.9, weight_decay=5e-4):
        dev = weights[0].device
        self.H, self.W = H, W
        self.wshapes = [tuple(w.shape) for w in weights]
        self.bshapes = [tuple(b.shape) for b in biases]
        self.opt_w = FlatOptimizer(sum(int(math.prod(s)) for s in self.wshapes), dev, optimizer, lr=lr, momentum=momentum, weight_decay=weight_decay)
        self.opt_b = FlatOptimizer(sum(int(math.prod(s)) for s in self.bshapes), dev, optimizer, lr=lr, momentum=momentum, weight_decay=0.0)
        self.w, self.dw = FlatOptimizer.views(self.opt_w.param, self.wshapes), FlatOptimizer.views(self.opt_w.grad, self.wshapes)
        self.b, self.db = FlatOptimizer.views(self.opt_b.param, self.bshapes), FlatOptimizer.views(self.opt_b.grad, self.bshapes)
        for dst, src in zip(self.w + self.b, list(weights) + list(biases)):
            dst.copy_(src)

    def forward_backward(self, x, target_ltrb, weight=None, target_scores_sum=1.0):
        """x bf16 [B,H,W,cin]; target_ltrb fp32 [B*H*W, 4] (bins), weight fp32 [B*H*W] or None -> (loss fp32[1], dx bf16 like x); the weight
        and bias gradients are left in the optimiser groups' gradient buffers (self.dw, self.db)."""
        H, W = self.H, self.W
        ks = [s[2] for s in self.wshapes]
        fw = [ops.conv_pack_bf16(w, H, W) for w in self.w]                       # this step's bf16 weights, forward order
        z1 = ops.conv_fwd_bf16(x, fw[0], self.b[0], self.wshapes[0][0], ks[0]); a1 = ops.silu_bf16(z1)
        z2 = ops.conv_fwd_bf16(a1, fw[1], self.b[1], self.wshapes[1][0], ks[1]); a2 = ops.silu_bf16(z2)
        out = ops.conv_fwd_bf16(a2, fw[2], self.b[2], self.wshapes[2][0], ks[2])
        loss, g = ops.dfl_loss(out.float().reshape(-1, self.wshapes[2][0]), target_ltrb, weight, target_scores_sum)
        d3 = g.reshape(out.shape).to(torch.bfloat16)
        bw = [ops.conv_pack_bf16(w, H, W, dgrad_form=True) for w in self.w]     # flipped / transposed: the input-gradient convolutions
        self.dw[2].copy_(ops.conv_wgrad_bf16(a2, d3, ks[2])); ops.bias_grad_bf16(d3, self.db[2])
        d2 = ops.silu_bwd_bf16(z2, ops.conv_fwd_bf16(d3, bw[2], None, self.wshapes[2][1], ks[2]))
        self.dw[1].copy_(ops.conv_wgrad_bf16(a1, d2, ks[1])); ops.bias_grad_bf16(d2, self.db[1])
        d1 = ops.silu_bwd_bf16(z1, ops.conv_fwd_bf16(d2, bw[1], None, self.wshapes[1][1], ks[1]))
        self.dw[0].copy_(ops.conv_wgrad_bf16(x, d1, ks[0])); ops.bias_grad_bf16(d1, self.db[0])
        dx = ops.conv_fwd_bf16(d1, bw[0], None, self.wshapes[0][1], ks[0])
        return loss, dx

    def step(self, x, target_ltrb, weight=None, target_scores_sum=1.0, group=None):
        loss, dx = self.forward_backward(x, target_ltrb, weight, target_scores_sum)
        allreduce_gradients([self.opt_w.grad, self.opt_b.grad], group)           # DDP: the gradient average (no-op on one rank)
        self.opt_w.step(); self.opt_b.step()
        return loss, dx


class ParamGroups:
    """The trainer's three optimiser groups (`param_group_of`: 0 = weights with decay, 1 = norm weights, 2 = biases; no decay in 1 and 2) as
    FlatOptimizers.  Layers `add` their initial tensors before `build()` allocates the flat buffers; afterwards `param[i]` / `grad[i]` are
    views of them, so the layers' kernels write gradients straight into the groups' gradient buffers.  A fourth flat buffer, `buffers`, holds the
    state that is no parameter (the BatchNorm running statistics, `add_buffer`): the EMA averages it with the weights, as the trainer's does."""

    def __init__(self, optimizer="SGD", lr=0.01, momentum=0.9, weight_decay=5e-4, nesterov=True, betas=None):
        self.cfg = dict(name=optimizer, lr=lr, momentum=momentum, nesterov=nesterov, betas=betas)
        self.weight_decay = weight_decay
        self.items, self.opts, self.param, self.grad = [], None, None, None
        self.buffer_items, self.buffers = [], None

    def add_buffer(self, t, owner, attr):
        """Register the fp32 tensor `t` = `owner.attr` as non-parameter state: `build()` moves its then-current value into the flat `buffers` and
        rebinds `owner.attr` to the view, so whatever reads or `copy_`s `owner.attr` before or after `build()` keeps working."""
        if self.opts is not None:
            raise RuntimeError("ParamGroups.add_buffer after build()")
        if getattr(owner, attr) is not t or t.dtype != torch.float32:
            raise ValueError("ParamGroups.add_buffer: t must be the fp32 tensor owner.attr")
        self.buffer_items.append((owner, attr))
        return len(self.buffer_items) - 1

    def add(self, group, init):
        if self.opts is not None:
            raise RuntimeError("ParamGroups.add after build()")
        self.items.append((int(group), init))
        return len(self.items) - 1

    def build(self):
        dev = self.items[0][1].device
        shapes = [[tuple(t.shape) for g, t in self.items if g == k] for k in range(3)]
        self.opts = [FlatOptimizer(sum(int(math.prod(s)) for s in shapes[k]), dev, weight_decay=self.weight_decay if k == 0 else 0.0, **self.cfg)
                     for k in range(3)]
        pv = [FlatOptimizer.views(o.param, sh) for o, sh in zip(self.opts, shapes)]
        gv = [FlatOptimizer.views(o.grad, sh) for o, sh in zip(self.opts, shapes)]
        self.param, self.grad, nxt = [], [], [0, 0, 0]
        for g, t in self.items:
            self.param.append(pv[g][nxt[g]]); self.grad.append(gv[g][nxt[g]])
            self.param[-1].copy_(t)
            nxt[g] += 1
        cur = [getattr(owner, attr) for owner, attr in self.buffer_items]
        self.buffers = torch.zeros(sum(t.numel() for t in cur), dtype=torch.float32, device=dev)
        for (owner, attr), t, v in zip(self.buffer_items, cur, FlatOptimizer.views(self.buffers, [tuple(t.shape) for t in cur])):
            v.copy_(t)
            setattr(owner, attr, v)
        return self

    def flat_grads(self):
        return [o.grad for o in self.opts if o.n]

    def step(self, lr=None, momentum=None, clip=None, grads=None):
        """The optimiser step of all three groups in ONE launch (ops.sgd_step_multi / adamw_step_multi; bit-identical to `FlatOptimizer.step` per
        group).  lr: None (each group's own), a number, or one per group (weights, norm weights, biases); momentum: None or this step's momentum
        (AdamW: betas[0]), as the warm-up sets them; clip: the fp32[3] device tensor of `clip_grad_norm` (the gradients are read times clip[1]) or
        None; grads: three flat buffers to step from in place of the groups' own (the accumulated gradients)."""
        opts = self.opts
        live = [o for o in opts if o.n]
        if not live:
            return
        if len({o.steps for o in live}) != 1:
            raise RuntimeError("ParamGroups.step: the groups' step counts differ (a group was stepped on its own)")
        lrs = [o.lr for o in opts] if lr is None else [lr] * 3 if isinstance(lr, (int, float)) else list(lr)
        if len(lrs) != 3:
            raise ValueError("ParamGroups.step: lr is a number or one per group (3)")
        grads = [o.grad for o in opts] if grads is None else list(grads)
        for o in live:
            o.steps += 1
        o0 = live[0]
        mu = o0.momentum if momentum is None else momentum
        wds = [o.weight_decay for o in opts]
        if o0.name == "SGD":
            ops.sgd_step_multi([o.param for o in opts], grads, [o.state[0] for o in opts], lrs, mu, wds, o0.nesterov, first_step=o0.steps == 1, clip=clip)
        else:
            betas = o0.betas if momentum is None else (momentum, o0.betas[1])
            ops.adamw_step_multi([o.param for o in opts], grads, [o.state[0] for o in opts], [o.state[1] for o in opts], o0.steps, lrs, betas, o0.eps, wds,
                                 clip=clip)


def wgrad_route(c1, c2):
    """Which block class of the weight-gradient kernel a dense conv c1 -> c2 runs in: "c64" when both channel counts are multiples of 64 (every
    block of dW is 64 x 64: the kernel instance with compile-time widths), "c8" for every other pair of multiples of 8 (some block at its
    live width).  Anything else is not a dense-kernel shape: the cin = 3 / 4 stem and the 12- and 1-channel head outputs have kernels of their
    own (StemConvBN, HeadOut; `train_kernel_of` routes every conv of the model)."""
    if c1 < 8 or c2 < 8 or c1 % 8 or c2 % 8:
        raise ValueError(f"wgrad_route: {c1} -> {c2}: channel counts must be multiples of 8, at least 8")
    return "c64" if c1 % 64 == 0 and c2 % 64 == 0 else "c8"


def conv_wgrad(x, dy, k, s=1, out=None):
    """dW of a dense conv at any channel counts `wgrad_route` accepts."""
    wgrad_route(x.shape[-1], dy.shape[-1])  # (ValueError for channel counts without a kernel)
    return ops.conv_wgrad_c8_bf16(x, dy, k, stride=s, out=out)


def train_kernel_of(k, s, g, c1, c2):
    """The kernel family that trains a conv layer (kernel k, stride s, groups g, c1 -> c2) of YOLO11-OBB:
        "dense"      ConvBN / the dense kernels, channel counts `wgrad_route` accepts, k 1 or 3 at stride 1, k 3 at stride 2;
        "depthwise"  DWConvBN: 3x3, stride 1, g = c1 = c2, a multiple of 8;
        "stem"       StemConvBN: 3x3, stride 2, c1 3 or 4 (the uint8 tile), c2 a multiple of 8 up to 64;
        "head_out"   HeadOut: 1x1, stride 1, c1 a multiple of 8 up to 512, 1 <= c2 <= 64 and c2 no multiple of 8.
    ValueError when no kernel exists."""
    if g == 1 and c1 >= 8 and c2 >= 8 and c1 % 8 == 0 and c2 % 8 == 0 and ((k in (1, 3) and s == 1) or (k == 3 and s == 2)):
        wgrad_route(c1, c2)
        return "dense"
    if g > 1 and g == c1 == c2 and c1 % 8 == 0 and k == 3 and s == 1:
        return "depthwise"
    if g == 1 and k == 3 and s == 2 and c1 in (3, 4) and c2 % 8 == 0 and 8 <= c2 <= 64:
        return "stem"
    if g == 1 and k == 1 and s == 1 and c1 % 8 == 0 and 8 <= c1 <= 512 and 1 <= c2 <= 64 and c2 % 8:
        return "head_out"
    raise ValueError(f"train_kernel_of: no training kernel for a {k}x{k} conv, stride {s}, groups {g}, {c1} -> {c2}")


class _BNBlock:
    """What ConvBN, DWConvBN and StemConvBN share: a conv without bias -> BatchNorm2d (batch statistics, running statistics updated) [-> SiLU] over
    fp32 master parameters held in `groups` (conv weight in group 0, gamma in 1, beta in 2; running statistics are buffers of the block, not
    parameters: `groups.add_buffer`).  `forward` is the subclass's `_conv_fwd`, then ops.bn_fwd_bf16; `backward` is ops.bn_bwd_bf16, then the subclass's `_conv_bwd`,
    which writes dW and returns dx.  A subclass checks its weight's shape, names (c1, c2, k, s, act) and supplies the two conv halves.  `g`: the
    conv's groups; `order`: None, or the row permutation `fold()` applies (a block held in another channel order than the checkpoint's)."""

    g, order = 1, None

    def __init__(self, groups, w, gamma, beta, c1, c2, k, s, act, running_mean, running_var, eps, momentum):
        self.c1, self.c2, self.k, self.s, self.act, self.eps, self.momentum = c1, c2, k, s, bool(act), eps, momentum
        dev = w.device
        self.groups = groups
        self._iw = groups.add(0, w)
        self._ig = groups.add(1, gamma if gamma is not None else torch.ones(c2, device=dev))
        self._ib = groups.add(2, beta if beta is not None else torch.zeros(c2, device=dev))
        self.running_mean = (running_mean.clone() if running_mean is not None else torch.zeros(c2, device=dev)).float().contiguous()
        self.running_var = (running_var.clone() if running_var is not None else torch.ones(c2, device=dev)).float().contiguous()
        groups.add_buffer(self.running_mean, self, "running_mean")  # (after build(): views of groups.buffers)
        groups.add_buffer(self.running_var, self, "running_var")
        self.saved = None

    w = property(lambda self: self.groups.param[self._iw])
    gamma = property(lambda self: self.groups.param[self._ig])
    beta = property(lambda self: self.groups.param[self._ib])
    dw = property(lambda self: self.groups.grad[self._iw])
    dgamma = property(lambda self: self.groups.grad[self._ig])
    dbeta = property(lambda self: self.groups.grad[self._ib])

    def forward(self, x):
        """x [B,H,W,c1] -> a bf16 [B,Ho,Wo,c2]; keeps (x, z, mean, invstd) for the backward."""
        z = self._conv_fwd(x)
        a, mean, invstd = ops.bn_fwd_bf16(z, self.gamma, self.beta, self.running_mean, self.running_var, self.eps, self.momentum, act=self.act)
        self.saved = (x, z, mean, invstd)
        return a

    def backward(self, da, **conv_args):
        """da bf16 like the forward's output -> dx bf16 like its input (or None: `_conv_bwd`); dW, dgamma, dbeta are written into the groups'
        gradient buffers."""
        x, z, mean, invstd = self.saved
        dz, _, _ = ops.bn_bwd_bf16(z, da, self.gamma, self.beta, mean, invstd, self.dgamma, self.dbeta, act=self.act)
        return self._conv_bwd(x, dz, **conv_args)

    def fold(self):
        """-> (w, b): the eval-mode BN folded into the conv (what model.fuse() and tools/export_obbw.py expect), fp32, rows in `order`."""
        f = self.gamma / torch.sqrt(self.running_var + self.eps)
        w, b = self.w * f.view(-1, 1, 1, 1), self.beta - self.running_mean * f
        return (w, b) if self.order is None else (w[self.order], b[self.order])


class ConvBN(_BNBlock):
    """ONE Ultralytics `Conv(c1, c2, k, s)` block in training mode -- Conv2d(bias=False) -> BatchNorm2d (batch statistics, running statistics
    updated) -> SiLU (act=False: no SiLU, Ultralytics' `Conv(..., act=False)`) -- on bf16 NHWC activations over fp32 master parameters held in `groups` (conv weight in group 0, gamma in 1, beta in 2).
    k = 1 or 3; s = 2 with k = 3 only (the downsampling convs).  Ultralytics' initialize_weights sets eps = 1e-3, momentum = 0.03 (recalled:
    the package is not installed here, so these defaults are unpinned like optimizer_config; both are arguments).  Every arithmetic step on
    the device is a libobbhip kernel; running statistics are buffers of the block, not parameters."""

    def __init__(self, groups, w, gamma=None, beta=None, s=1, running_mean=None, running_var=None, eps=1e-3, momentum=0.03, act=True):
        c2, c1, k, k2 = w.shape
        if k != k2 or k not in (1, 3) or s not in (1, 2) or (s == 2 and k != 3):
            raise ValueError(f"ConvBN: k = {k}, s = {s}: k 1 or 3 at stride 1, k 3 at stride 2")
        super().__init__(groups, w, gamma, beta, c1, c2, k, s, act, running_mean, running_var, eps, momentum)

    pack = None  # the PackPlan that holds this layer's packed weights, once one is attached (then nothing is packed per call)

    def _packed(self, H, W, dgrad_form=False):
        """This step's bf16 weights for H x W input maps: a view of the attached plan's buffer (the consuming op checks its length with
        ops._check_packed), or packed here, per call."""
        if self.pack is not None:
            return self.pack.view(self, H, W, dgrad_form)
        return ops.conv_pack_bf16(self.w, H, W, dgrad_form=True) if dgrad_form else ops.conv_pack_bf16(self.w, H, W, stride=self.s)

    def _conv_fwd(self, x):
        return ops.conv_fwd_bf16(x, self._packed(x.shape[1], x.shape[2]), None, self.c2, self.k, stride=self.s)

    def _conv_bwd(self, x, dz):
        H, W = x.shape[1], x.shape[2]
        conv_wgrad(x, dz, self.k, self.s, out=self.dw)
        bw = self._packed(H, W, dgrad_form=True)
        if self.s == 2:
            return ops.conv_dgrad_s2_bf16(dz, bw, self.c1, H, W)
        return ops.conv_fwd_bf16(dz, bw, None, self.c1, self.k)


class DWConvBN(_BNBlock):
    """ONE depthwise Ultralytics block in training mode -- `DWConv(c, c, 3)` = Conv2d(c, c, 3, 1, 1, groups=c, bias=False) -> BatchNorm2d -> SiLU
    (act=True: the head's class branch, model.23.cv3.i.{0,1}.0) or without the SiLU (act=False: `Conv(c, c, 3, g=c, act=False)`, C2PSA's
    attn.pe) -- under ConvBN's contract: bf16 NHWC activations, fp32 master parameters in `groups` (w [C,1,3,3] in group 0, gamma in 1, beta in
    2), `forward` / `backward` / `fold`.  The kernels read the master weights directly (rounded to bf16 as they are loaded: no pack step); the
    backward takes dx and dW from one pass over x and dz, dW written straight into the group's gradient view (`backward(da, need_dx=False)`:
    dW alone, None returned)."""

    def __init__(self, groups, w, gamma=None, beta=None, act=True, running_mean=None, running_var=None, eps=1e-3, momentum=0.03):
        if w.dim() != 4 or tuple(w.shape[1:]) != (1, 3, 3):
            raise ValueError(f"DWConvBN: w must be the depthwise 3x3 weights [C,1,3,3], got {tuple(w.shape)}")
        super().__init__(groups, w, gamma, beta, w.shape[0], w.shape[0], 3, 1, act, running_mean, running_var, eps, momentum)

    g = property(lambda self: self.c1)

    def _conv_fwd(self, x):
        return ops.dwconv3_fwd_bf16(x, self.w)

    def _conv_bwd(self, x, dz, need_dx=True):
        dx, _ = ops.dwconv3_bwd_bf16(x, dz, self.w, dw_out=self.dw, need_dx=need_dx)
        return dx


def _bn_block(cls, groups, t, eps, momentum, **kw):
    """t = (w, gamma, beta[, running_mean, running_var]), gamma / beta None: 1 / 0 -> cls(groups, ...), cls a _BNBlock; kw: its `s` or `act`."""
    w, gamma, beta, running_mean, running_var = (tuple(t) + (None,) * 4)[:5]
    return cls(groups, w, gamma, beta, running_mean=running_mean, running_var=running_var, eps=eps, momentum=momentum, **kw)


class _Composite:
    """A module that owns layers states them ONCE: `children()` -> [(checkpoint-relative name, child)] in checkpoint order, a child being a leaf
    (a _BNBlock or a _ConvBias: a layer with parameters of its own, no children) or another _Composite.  Everything that needs "every layer
    under its name" is this one walk."""

    def named_blocks(self):
        """[(checkpoint-relative name, leaf)]: the children flattened, names joined with "." -- registration order, but for a DetectHead on groups
        of its own"""
        return [nb for name, c in self.children() for nb in _flatten(name, c)]

    def fold(self):
        """-> {name: (w, b)} per leaf of named_blocks(): eval-mode BN folded into each conv, fp32, checkpoint channel order."""
        return {name: b.fold() for name, b in self.named_blocks()}


def _flatten(name, m):
    """[(name, leaf)] of the subtree `m` that its parent lists as `name`"""
    return [(f"{name}.{n}", b) for n, b in m.named_blocks()] if isinstance(m, _Composite) else [(name, m)]


class _Chain(_Composite):
    """Layers in a row, `self.chain`: forward through them in order, backward through them reversed; the checkpoint names them 0, 1, ..."""

    def children(self):
        return [(str(j), m) for j, m in enumerate(self.chain)]

    def forward(self, x):
        for m in self.chain:
            x = m.forward(x)
        return x

    def backward(self, d):
        for m in reversed(self.chain):
            d = m.backward(d)
        return d


class ClassBranchPair(_Chain):
    """One `Sequential(DWConv(c1, c1, 3), Conv(c1, c2, 1))` of the head's class branch (ultralytics Detect.cv3[i][0] and [1]; the branch is two
    such pairs and the nc-channel logit Conv2d) in training mode: DWConvBN -> ConvBN(1x1), both with SiLU.  dw / pw: (w, gamma, beta[,
    running_mean, running_var]) of the two blocks, registered in `groups` in that order.  forward(x bf16 [B,H,W,c1]) -> bf16 [B,H,W,c2];
    backward(da) -> dx, the six parameter gradients written into the groups' gradient buffers."""

    def __init__(self, groups, dw, pw, eps=1e-3, momentum=0.03):
        self.dw = _bn_block(DWConvBN, groups, dw, eps, momentum)
        self.pw = _bn_block(ConvBN, groups, pw, eps, momentum)
        if self.pw.k != 1 or self.pw.c1 != self.dw.c2:
            raise ValueError(f"ClassBranchPair: pw is a 1x1 conv reading dw's {self.dw.c2} channels, got k = {self.pw.k}, c1 = {self.pw.c1}")
        self.chain = [self.dw, self.pw]


def qkv_device_order(nh, kd=32, hd=64):
    """-> LongTensor perm: device channel i of the qkv conv is checkpoint channel perm[i].  The checkpoint groups the output channels per head,
    [q | k | v] of head 0, then head 1, ...; the attention kernels read [q of all heads | k of all heads | v of all heads], so that v is one
    contiguous slice (the permutation the forward engine applies to the same layer at load)."""
    perm = []
    for off, n in ((0, kd), (kd, kd), (2 * kd, hd)):
        for h in range(nh):
            perm.extend(range(h * (2 * kd + hd) + off, h * (2 * kd + hd) + off + n))
    return torch.tensor(perm, dtype=torch.long)


class Attention(_Composite):
    """Ultralytics `Attention(dim, num_heads, attn_ratio=0.5)` (model.10.m.i.attn; key_dim 32, head_dim 64, nh = dim / 64) in training mode:
        qkv = Conv 1x1 (dim -> 2 dim, no act);  out = softmax(scale q^T k) applied to v per head;  y = proj(out + pe(v)),
    pe = depthwise Conv 3x3 (no act), proj = Conv 1x1 (no act).  qkv / proj / pe: (w, gamma, beta[, running_mean, running_var]) of the three
    blocks in CHECKPOINT channel order, registered in `groups` in that order.  The qkv block is HELD in device order (`qkv_device_order`: its
    rows of w, gamma, beta and the running statistics are permuted once, here), so its parameters, gradients and running statistics in `groups`
    are in device order; its `order` is set, so that its `fold()` hands the rows back in checkpoint order.  The v slice of qkv that pe reads is
    a channel-window copy (ops.chanwin_bf16).  bf16 [B,H,W,dim] in and out, H W <= 192."""

    def __init__(self, groups, qkv, proj, pe, nh, eps=1e-3, momentum=0.03):
        self.nh = int(nh)
        dim = self.nh * 64
        if tuple(qkv[0].shape) != (2 * dim, dim, 1, 1) or tuple(proj[0].shape) != (dim, dim, 1, 1) or tuple(pe[0].shape) != (dim, 1, 3, 3):
            raise ValueError(f"Attention: nh = {nh} heads of 64 channels: qkv [{2 * dim},{dim},1,1], proj [{dim},{dim},1,1], pe [{dim},1,3,3], got "
                             f"{tuple(qkv[0].shape)}, {tuple(proj[0].shape)}, {tuple(pe[0].shape)}")
        self.perm = qkv_device_order(self.nh).to(qkv[0].device)
        self.inv = torch.argsort(self.perm)
        self.qkv = _bn_block(ConvBN, groups, [None if t is None else t[self.perm].contiguous() for t in qkv], eps, momentum, act=False)
        self.qkv.order = self.inv
        self.proj = _bn_block(ConvBN, groups, proj, eps, momentum, act=False)
        self.pe = _bn_block(DWConvBN, groups, pe, eps, momentum, act=False)
        self.saved = None

    def forward(self, x):
        """x bf16 [B,H,W,dim] -> bf16 [B,H,W,dim]; keeps (qkv, out, lse) for the backward."""
        qkv = self.qkv.forward(x)
        out, lse = ops.attn_fwd_bf16(qkv, self.nh)
        v = ops.chanwin_bf16(qkv, self.nh * 64, self.nh * 64)
        self.saved = (qkv, out, lse)
        return self.proj.forward(ops.add_bf16(out, self.pe.forward(v)))

    def backward(self, dy):
        """dy bf16 like the forward's output -> dx bf16 like its input; the nine parameter gradients go into the groups' gradient buffers.  The
        gradient of `out + pe(v)` goes to both the core and pe; pe's dx arrives in dV inside the core's backward (dv_add)."""
        qkv, out, lse = self.saved
        ds = self.proj.backward(dy)
        dqkv = ops.attn_bwd_bf16(qkv, out, lse, ds, self.nh, dv_add=self.pe.backward(ds))
        return self.qkv.backward(dqkv)

    def children(self):
        return [("qkv", self.qkv), ("proj", self.proj), ("pe", self.pe)]


class PSABlock(_Composite):
    """Ultralytics `PSABlock(c, attn_ratio=0.5, num_heads=c // 64)` (model.10.m.i) in training mode:
        x = x + attn(x);  x = x + ffn1(ffn0(x)),   ffn0 = Conv 1x1 (c -> 2 c, SiLU), ffn1 = Conv 1x1 (2 c -> c, no act).
    qkv / proj / pe as for `Attention`, ffn0 / ffn1: (w, gamma, beta[, running_mean, running_var]); registered in `groups` in the order qkv,
    proj, pe, ffn0, ffn1.  The two residual adds and the two gradient sums at their fan-outs are ops.add_bf16 (fp32 add, one rounding)."""

    def __init__(self, groups, qkv, proj, pe, ffn0, ffn1, nh, eps=1e-3, momentum=0.03):
        self.attn = Attention(groups, qkv, proj, pe, nh, eps, momentum)
        self.ffn0 = _bn_block(ConvBN, groups, ffn0, eps, momentum)
        self.ffn1 = _bn_block(ConvBN, groups, ffn1, eps, momentum, act=False)
        c = self.attn.nh * 64
        if (self.ffn0.k, self.ffn0.c1, self.ffn1.k, self.ffn1.c1, self.ffn1.c2) != (1, c, 1, self.ffn0.c2, c):
            raise ValueError(f"PSABlock: ffn0 and ffn1 are 1x1 convs {c} -> m -> {c}, got {tuple(ffn0[0].shape)}, {tuple(ffn1[0].shape)}")

    NAMES = ("attn.qkv", "attn.proj", "attn.pe", "ffn.0", "ffn.1")  # the checkpoint's names of the constructor's five blocks, in its order

    def children(self):
        return [("attn", self.attn), ("ffn.0", self.ffn0), ("ffn.1", self.ffn1)]

    def forward(self, x):
        """x bf16 [B,H,W,c] -> bf16 [B,H,W,c]."""
        x1 = ops.add_bf16(x, self.attn.forward(x))
        return ops.add_bf16(x1, self.ffn1.forward(self.ffn0.forward(x1)))

    def backward(self, dy):
        """dy bf16 like the forward's output -> dx bf16 like its input; the fifteen parameter gradients go into the groups' gradient buffers."""
        d1 = ops.add_bf16(dy, self.ffn0.backward(self.ffn1.backward(dy)))
        return ops.add_bf16(d1, self.attn.backward(d1))


class SPPF(_Composite):
    """Ultralytics `SPPF(c1, c2, k=5)` (yolo11 model 9) in training mode: cv1 = Conv 1x1 (c1 -> c1 / 2), three chained 5x5 max pools (stride 1,
    pad 2), cv2 = Conv 1x1 over cat([a1, y1, y2, y3]) (2 c1 -> c2).  cv1 / cv2: (w, gamma, beta[, running_mean, running_var]) of the two ConvBN
    blocks, registered in `groups` in that order.  `forward` / `backward` follow ConvBN's contract; the only tensor kept for the pools' backward
    is `cat` (cv2's input, kept for its wgrad anyway): the argmax is recomputed from it (csrc/routegrad.hip).  Maps up to 32 x 32."""

    def __init__(self, groups, cv1, cv2, eps=1e-3, momentum=0.03):
        self.cv1, self.cv2 = _bn_block(ConvBN, groups, cv1, eps, momentum), _bn_block(ConvBN, groups, cv2, eps, momentum)
        if self.cv1.k != 1 or self.cv2.k != 1 or self.cv2.c1 != 4 * self.cv1.c2:
            raise ValueError(f"SPPF: cv1 and cv2 are 1x1 convs with cv2 reading 4 x cv1's {self.cv1.c2} channels, got k = {self.cv1.k}, {self.cv2.k}, "
                             f"cv2 c1 = {self.cv2.c1}")
        self.cat = None

    def children(self):
        return [("cv1", self.cv1), ("cv2", self.cv2)]

    def forward(self, x):
        """x bf16 [B,H,W,c1] -> bf16 [B,H,W,c2]."""
        self.cat = ops.sppf_pools_fwd_bf16(self.cv1.forward(x))
        return self.cv2.forward(self.cat)

    def backward(self, da):
        """da bf16 like the forward's output -> dx bf16 like its input; the six parameter gradients go into the groups' gradient buffers."""
        return self.cv1.backward(ops.sppf_pools_bwd_bf16(self.cat, self.cv2.backward(da)))


class UpCat:
    """`nn.Upsample(scale_factor=up, mode="nearest")` + `Concat([-1, skip])` of the FPN (up = 2; yolo11 models 11/12, 14/15) or the plain
    `Concat` of the PAN (up = 1; models 18, 21): forward(a, b) = cat(upsample(a), b) along C.  backward(dout, da, db) -> (da, db): a given
    da / db already holds the gradient of that tensor's other consumer and is added to (fp32 add, one bf16 rounding); None allocates."""

    def __init__(self, up=1):
        if up not in (1, 2):
            raise ValueError(f"UpCat: up = {up}: 1 (concat) or 2 (upsample + concat)")
        self.up, self.ca = up, None

    def forward(self, a, b):
        self.ca = a.shape[-1]
        return ops.upcat_fwd_bf16(a, b, self.up)

    def backward(self, dout, da=None, db=None):
        return ops.upcat_bwd_bf16(dout, self.ca, self.up, da=da, db=db)


class Bottleneck(_Composite):
    """Ultralytics `Bottleneck(c1, c2, shortcut=True, k=(3, 3), e)` with c1 == c2 (every use in YOLO11) in training mode: out = x + cv2(cv1(x)), two
    3x3 ConvBN.  cv1 / cv2: (w, gamma, beta[, running_mean, running_var]), registered in `groups` in that order.  The residual add and the gradient
    sum at x's fan-out are ops.add_bf16 (fp32 add, one rounding).  ConvBN's contract: bf16 NHWC in and out, `forward` / `backward` / `fold`."""

    def __init__(self, groups, cv1, cv2, eps=1e-3, momentum=0.03):
        self.cv1, self.cv2 = _bn_block(ConvBN, groups, cv1, eps, momentum), _bn_block(ConvBN, groups, cv2, eps, momentum)
        if (self.cv1.k, self.cv2.k) != (3, 3) or self.cv2.c1 != self.cv1.c2 or self.cv2.c2 != self.cv1.c1:
            raise ValueError(f"Bottleneck: cv1 and cv2 are 3x3 convs c -> c_ -> c (the shortcut is always taken), got {tuple(cv1[0].shape)}, "
                             f"{tuple(cv2[0].shape)}")
        self.c1 = self.c2 = self.cv1.c1

    def children(self):
        return [("cv1", self.cv1), ("cv2", self.cv2)]

    def forward(self, x):
        """x bf16 [B,H,W,c] -> bf16 [B,H,W,c]."""
        return ops.add_bf16(x, self.cv2.forward(self.cv1.forward(x)))

    def backward(self, dy):
        """dy bf16 like the forward's output -> dx bf16 like its input; the six parameter gradients go into the groups' gradient buffers."""
        return ops.add_bf16(dy, self.cv1.backward(self.cv2.backward(dy)))


class C3k(_Composite):
    """Ultralytics `C3k(c1, c2, n, e=0.5, k=3)` (the members of the deeper C3k2 blocks) in training mode: cv3(cat(m(cv1(x)), cv2(x))), cv1 / cv2 =
    Conv 1x1 (c1 -> c_), m = n Bottlenecks c_ -> c_ -> c_ (e = 1.0), cv3 = Conv 1x1 (2 c_ -> c2).  cv1 / cv2 / cv3: parameter tuples as for
    Bottleneck; m: a list of (cv1, cv2) pairs.  Registered in `groups` in the order cv1, cv2, cv3, m.0.cv1, m.0.cv2, m.1.cv1, ...  The concat and
    its backward are the upcat ops with up = 1; the two gradients of x are summed by ops.add_bf16."""

    def __init__(self, groups, cv1, cv2, cv3, m, eps=1e-3, momentum=0.03):
        self.cv1, self.cv2, self.cv3 = (_bn_block(ConvBN, groups, t, eps, momentum) for t in (cv1, cv2, cv3))
        self.m = [Bottleneck(groups, a, b, eps, momentum) for (a, b) in m]
        c_ = self.cv1.c2
        if (self.cv1.k, self.cv2.k, self.cv3.k) != (1, 1, 1) or self.cv2.c1 != self.cv1.c1 or self.cv2.c2 != c_ or self.cv3.c1 != 2 * c_:
            raise ValueError(f"C3k: cv1, cv2 are 1x1 convs c1 -> c_ and cv3 a 1x1 conv 2 c_ -> c2, got {tuple(cv1[0].shape)}, {tuple(cv2[0].shape)}, "
                             f"{tuple(cv3[0].shape)}")
        if not self.m or any(b.c1 != c_ for b in self.m):
            raise ValueError(f"C3k: m is at least one Bottleneck on cv1's {c_} channels, got {[b.c1 for b in self.m]}")
        self.c1, self.c2, self.c_ = self.cv1.c1, self.cv3.c2, c_

    def children(self):
        return [("cv1", self.cv1), ("cv2", self.cv2), ("cv3", self.cv3)] + [(f"m.{i}", m) for i, m in enumerate(self.m)]

    def forward(self, x):
        """x bf16 [B,H,W,c1] -> bf16 [B,H,W,c2]."""
        a = self.cv1.forward(x)
        for m in self.m:
            a = m.forward(a)
        return self.cv3.forward(ops.upcat_fwd_bf16(a, self.cv2.forward(x), 1))

    def backward(self, dy):
        """dy bf16 like the forward's output -> dx bf16 like its input; every parameter gradient goes into the groups' gradient buffers."""
        da, db = ops.upcat_bwd_bf16(self.cv3.backward(dy), self.c_, 1)
        for m in reversed(self.m):
            da = m.backward(da)
        return ops.add_bf16(self.cv1.backward(da), self.cv2.backward(db))


class C3k2(_Composite):
    """Ultralytics `C3k2(c1, c2, n, c3k, e)` (yolo11 models 2, 4, 6, 8, 13, 16, 19, 22) in training mode, any n >= 1:
        t = cv1(x) (2 c channels);  y0, y1 = t.chunk(2);  y_{i+2} = m_i(y_{i+1});  out = cv2(cat(y0, y1, y2, ..., y_{n+1})),
    cv1 = Conv 1x1 (c1 -> 2 c), cv2 = Conv 1x1 ((2 + n) c -> c2), m_i = Bottleneck c -> c/2 -> c (c3k False; m: a list of (cv1, cv2) pairs) or
    C3k c -> c (c3k True; m: a list of (cv1, cv2, cv3, [(cv1, cv2), ...])).  Registered in `groups` in the order cv1, cv2, then the members.
    `cat` is allocated once and every member is written into its channel window (ops.chanwin_bf16: bit copies); in the backward the gradient of
    y_i is dcat's window i plus the gradient that comes back through m_i, one window add (fp32, one rounding) per member."""

    def __init__(self, groups, cv1, cv2, m, c3k=False, eps=1e-3, momentum=0.03):
        self.cv1, self.cv2 = _bn_block(ConvBN, groups, cv1, eps, momentum), _bn_block(ConvBN, groups, cv2, eps, momentum)
        self.m = [C3k(groups, *t, eps, momentum) if c3k else Bottleneck(groups, *t, eps, momentum) for t in m]
        n, c = len(self.m), self.cv1.c2 // 2
        if (self.cv1.k, self.cv2.k) != (1, 1) or self.cv1.c2 % 16 or n < 1 or self.cv2.c1 != (2 + n) * c:
            raise ValueError(f"C3k2: cv1 is a 1x1 conv c1 -> 2 c (c a multiple of 8) and cv2 a 1x1 conv (2 + n) c -> c2 over n = {n} members, got "
                             f"{tuple(cv1[0].shape)}, {tuple(cv2[0].shape)}")
        if any(b.c1 != c or b.c2 != c for b in self.m):
            raise ValueError(f"C3k2: every member maps c = {c} channels to c, got {[(b.c1, b.c2) for b in self.m]}")
        self.c1, self.c2, self.c = self.cv1.c1, self.cv2.c2, c

    def children(self):
        return [("cv1", self.cv1), ("cv2", self.cv2)] + [(f"m.{i}", m) for i, m in enumerate(self.m)]

    def forward(self, x):
        """x bf16 [B,H,W,c1] -> bf16 [B,H,W,c2]."""
        c, n = self.c, len(self.m)
        t = self.cv1.forward(x)
        cat = torch.empty((*t.shape[:-1], (2 + n) * c), dtype=torch.bfloat16, device=t.device)
        ops.chanwin_bf16(t, 0, 2 * c, dst=cat, d0=0)
        y = ops.chanwin_bf16(t, c, c)
        for i, m in enumerate(self.m):
            y = m.forward(y)
            ops.chanwin_bf16(y, 0, c, dst=cat, d0=(2 + i) * c)
        return self.cv2.forward(cat)

    def backward(self, dy):
        """dy bf16 like the forward's output -> dx bf16 like its input; every parameter gradient goes into the groups' gradient buffers."""
        c, n = self.c, len(self.m)
        dcat = self.cv2.backward(dy)
        g = ops.chanwin_bf16(dcat, (1 + n) * c, c)
        for i in range(n, 0, -1):
            g = ops.chanwin_bf16(dcat, i * c, c, add=self.m[i - 1].backward(g))
        dt = torch.empty((*dcat.shape[:-1], 2 * c), dtype=torch.bfloat16, device=dcat.device)
        ops.chanwin_bf16(dcat, 0, c, dst=dt, d0=0)
        ops.chanwin_bf16(g, 0, c, dst=dt, d0=c)
        return self.cv1.backward(dt)


class C2PSA(_Composite):
    """Ultralytics `C2PSA(c1, c1, n, e=0.5)` (yolo11 model 10) in training mode: a, b = cv1(x).split((c, c));  b = m(b);  out = cv2(cat(a, b)),
    cv1 = Conv 1x1 (c1 -> 2 c), cv2 = Conv 1x1 (2 c -> c1), m = n PSABlocks on c = 64 nh channels.  cv1 / cv2: parameter tuples as for Bottleneck;
    blocks: a list of (qkv, proj, pe, ffn0, ffn1) as `PSABlock` takes them (`PSABlock.NAMES`).  Registered in `groups` in the order cv1, cv2, then
    the blocks.  The split is two channel-window copies, the concat and its backward the upcat ops with up = 1; dt = cat(da, db') again by upcat."""

    def __init__(self, groups, cv1, cv2, blocks, nh, eps=1e-3, momentum=0.03):
        self.cv1, self.cv2 = _bn_block(ConvBN, groups, cv1, eps, momentum), _bn_block(ConvBN, groups, cv2, eps, momentum)
        self.m = [PSABlock(groups, *t, nh, eps, momentum) for t in blocks]
        c = int(nh) * 64
        if (self.cv1.k, self.cv2.k) != (1, 1) or self.cv1.c2 != 2 * c or self.cv2.c1 != 2 * c or not self.m:
            raise ValueError(f"C2PSA: nh = {nh} heads of 64 channels: cv1 is a 1x1 conv c1 -> {2 * c}, cv2 a 1x1 conv {2 * c} -> c2 around at least one "
                             f"PSABlock, got {tuple(cv1[0].shape)}, {tuple(cv2[0].shape)}, {len(self.m)} blocks")
        self.c1, self.c2, self.c = self.cv1.c1, self.cv2.c2, c

    def children(self):
        return [("cv1", self.cv1), ("cv2", self.cv2)] + [(f"m.{i}", m) for i, m in enumerate(self.m)]

    def forward(self, x):
        """x bf16 [B,H,W,c1] -> bf16 [B,H,W,c2]; H W <= 192 (the attention core)."""
        t = self.cv1.forward(x)
        a, b = ops.chanwin_bf16(t, 0, self.c), ops.chanwin_bf16(t, self.c, self.c)
        for m in self.m:
            b = m.forward(b)
        return self.cv2.forward(ops.upcat_fwd_bf16(a, b, 1))

    def backward(self, dy):
        """dy bf16 like the forward's output -> dx bf16 like its input; every parameter gradient goes into the groups' gradient buffers."""
        da, db = ops.upcat_bwd_bf16(self.cv2.backward(dy), self.c, 1)
        for m in reversed(self.m):
            db = m.backward(db)
        return self.cv1.backward(ops.upcat_fwd_bf16(da, db, 1))


class StemConvBN(_BNBlock):
    """model.0 in training mode -- Conv2d(cin, c2, 3, 2, 1, bias=False) on the uint8 NHWC tile [B,H,W,cin] (cin 3 or 4, the operand is bf16(v / 255),
    channel order as stored) -> BatchNorm2d (batch statistics) -> SiLU -- under ConvBN's contract and parameter groups (w [c2,cin,3,3] in group 0,
    gamma in 1, beta in 2, running statistics as buffers).  The conv kernels read the tile and the master weights directly (csrc/narrowgrad.hip:
    no float copy of the image, no pack step).  forward(x uint8 [B,H,W,cin]) -> bf16 [B,(H+1)//2,(W+1)//2,c2]; `backward` returns None: the input is
    the image.  `fold()`: the weights of a conv on v / 255."""

    def __init__(self, groups, w, gamma=None, beta=None, running_mean=None, running_var=None, eps=1e-3, momentum=0.03):
        if w.dim() != 4 or w.shape[1] not in (3, 4) or tuple(w.shape[2:]) != (3, 3) or w.shape[0] % 8 or not 8 <= w.shape[0] <= 64:
            raise ValueError(f"StemConvBN: w must be [c2,3 or 4,3,3] with c2 a multiple of 8 in [8, 64], got {tuple(w.shape)}")
        super().__init__(groups, w, gamma, beta, w.shape[1], w.shape[0], 3, 2, True, running_mean, running_var, eps, momentum)

    def _conv_fwd(self, x):
        return ops.stemconv_fwd_u8(x, self.w)

    def _conv_bwd(self, x, dz):
        ops.stemconv_wgrad_u8(x, dz, out=self.dw)
        return None


class _ConvBias:
    """A plain 1x1 `nn.Conv2d` with bias at the end of a head branch: w [cout,c,1,1] in group 0 of `groups`, b [cout] in group 2."""

    k, s, g, act = 1, 1, 1, False

    def __init__(self, groups, w, b):
        self.c2, self.c1 = w.shape[0], w.shape[1]
        self.groups = groups
        self._iw, self._ib = groups.add(0, w), groups.add(2, b)
        self.saved = None

    w = property(lambda self: self.groups.param[self._iw])
    b = property(lambda self: self.groups.param[self._ib])
    dw = property(lambda self: self.groups.grad[self._iw])
    db = property(lambda self: self.groups.grad[self._ib])

    def fold(self):
        """-> (w, b) as they are: there is no BatchNorm to fold"""
        return self.w, self.b


class HeadOut(_ConvBias):
    """A plain `nn.Conv2d(c, cout, 1)` with bias at the end of a head branch (model.23.cv3.i.2: nc class logits; model.23.cv4.i.2: the angle logit)
    in training mode: w [cout,c,1,1] in group 0, b [cout] in group 2.  forward(x bf16 [B,H,W,c]) -> FP32 logits [B,H,W,cout] (what the losses
    read); backward(dy fp32) -> dx bf16, with dW and db written straight into the groups' gradient views by the same pass (csrc/narrowgrad.hip)."""

    def __init__(self, groups, w, b):
        if w.dim() != 4 or tuple(w.shape[2:]) != (1, 1) or b.dim() != 1 or b.shape[0] != w.shape[0]:
            raise ValueError(f"HeadOut: w must be [cout,c,1,1] and b [cout], got {tuple(w.shape)}, {tuple(b.shape)}")
        c2, c1 = w.shape[0], w.shape[1]
        if c1 % 8 or not 8 <= c1 <= 512 or not 1 <= c2 <= 64:
            raise ValueError(f"HeadOut: {c1} -> {c2}: c a multiple of 8 in [8, 512], 1 <= cout <= 64")
        super().__init__(groups, w, b)

    def forward(self, x):
        self.saved = x
        return ops.headconv_fwd_bf16(x, self.w, self.b)

    def backward(self, dy, need_dx=True):
        dx, _, _ = ops.headconv_bwd_bf16(self.saved, dy, self.w, dw_out=self.dw, db_out=self.db, need_dx=need_dx)
        return dx


class BoxOut(_ConvBias):
    """The box branch's output (model.23.cv2.i.2: 4 x 16 DFL logits, a multiple of 8 channels) under HeadOut's contract, on the dense kernels and
    with BF16 logits: forward(x bf16 [B,H,W,c]) -> bf16 [B,H,W,cout] = pack + conv + bias; backward(dy bf16) -> dx bf16 = weight gradient and bias
    gradient into the groups' gradient views, then the conv on the dgrad-form pack."""

    pack = None  # (as ConvBN's)

    def _packed(self, H, W, dgrad_form=False):
        if self.pack is not None:
            return self.pack.view(self, H, W, dgrad_form)
        return ops.conv_pack_bf16(self.w, H, W, dgrad_form=dgrad_form)

    def forward(self, x):
        self.saved = x
        return ops.conv_fwd_bf16(x, self._packed(x.shape[1], x.shape[2]), self.b, self.c2, 1)

    def backward(self, dy):
        x = self.saved
        conv_wgrad(x, dy, 1, out=self.dw)
        ops.bias_grad_bf16(dy, self.db)
        return ops.conv_fwd_bf16(dy, self._packed(x.shape[1], x.shape[2], dgrad_form=True), None, self.c1, 1)


class _DetectBoxBranch(_Chain):
    """Detect.cv2[i]: ConvBN 3x3 -> ConvBN 3x3 -> `OUT` = BoxOut -> bf16 [B,H,W,64] DFL logits.  convs: two (w, gamma, beta) triples (gamma / beta
    None: 1 / 0), registered in `groups` before w3 [c_out,c,1,1] (group 0) and b3 [c_out] (group 2), which read through as w3 / b3 / dw3 / db3."""
    OUT = BoxOut

    def __init__(self, groups, convs, w3, b3, eps=1e-3, momentum=0.03):
        self.blocks = [_bn_block(ConvBN, groups, t, eps, momentum) for t in convs]
        self.out = self.OUT(groups, w3, b3)
        self.chain = self.blocks + [self.out]

    w3 = property(lambda self: self.out.w)
    b3 = property(lambda self: self.out.b)
    dw3 = property(lambda self: self.out.dw)
    db3 = property(lambda self: self.out.db)
    cout3 = property(lambda self: self.out.c2)


class _DetectClassBranch(_Chain):
    """Detect.cv3[i]: two ClassBranchPairs (DWConv 3x3 -> Conv 1x1, BatchNorm unfolded) -> HeadOut(nc) -> fp32 class logits.  pairs: two (dw, pw)
    with dw / pw = (w, gamma, beta[, running_mean, running_var]), registered in `groups` before w3 [nc,c,1,1] and b3 [nc]."""

    def __init__(self, groups, pairs, w3, b3, eps, momentum):
        self.pairs = [ClassBranchPair(groups, dw, pw, eps, momentum) for (dw, pw) in pairs]
        self.out = HeadOut(groups, w3, b3)
        self.chain = self.pairs + [self.out]


class DetectAngleBranch(_DetectBoxBranch):
    """Ultralytics OBB.cv4[i]: the box branch's chain ending in HeadOut(1): forward(x bf16) -> fp32 angle logits [B,H,W,1], backward(dangle fp32) ->
    dx bf16.  There is no loss here: the angle's gradient arrives through ProbIoU on the decoded boxes.  w3 [ne,c,1,1], b3 [ne]."""
    OUT = HeadOut


class _Step:
    """step(*inputs, group=None) of a module with `forward_backward(*inputs)` and `groups`: forward + backward, the DDP gradient average over
    `group` (no-op on one rank), the optimiser step -> what forward_backward returned.  With `update` set (a `TrainerUpdate` over the same groups)
    everything after the backward is the trainer's: step(*inputs, ni=, epoch=) hands it the iteration and epoch numbers, and `last_clip` keeps what
    it returned (the clip tensor, or None between two optimiser steps of an accumulation)."""
    update = None

    def step(self, *inputs, group=None, ni=None, epoch=None, **kw):
        if self.update is None:
            if ni is not None or epoch is not None:
                raise TypeError("step: ni / epoch are the iteration and epoch of a TrainerUpdate, and `update` is not set")
            out = self.forward_backward(*inputs, **kw)
            allreduce_gradients(self.groups.flat_grads(), group)
            self.groups.step()
            return out
        if ni is None or epoch is None:
            raise TypeError("step: with `update` set, pass ni= and epoch= (the schedule needs them)")
        out = self.forward_backward(*inputs, **kw)
        self.last_clip = self.update(ni, epoch, group=group)
        return out


class _BranchStep(_Step):
    """A head branch (`BRANCH`) on the trainer's three parameter groups of its own, trained under one term of the loss by the subclass's
    `forward_backward`.  The branch's attributes (its layers and their parameter views) read through."""

    def __init__(self, layers, w3, b3, optimizer="SGD", lr=0.01, momentum=0.9, weight_decay=5e-4, nesterov=True, eps=1e-3, bn_momentum=0.03):
        self.groups = ParamGroups(optimizer, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov)
        self.branch = self.BRANCH(self.groups, layers, w3, b3, eps, bn_momentum)
        self.groups.build()

    def __getattr__(self, name):
        if name == "branch":  # (not built yet)
            raise AttributeError(name)
        return getattr(self.branch, name)


class DetectBoxBranchStep(_BranchStep):
    """Ultralytics Detect.cv2[i] trained as the reference trains it, BatchNorm UNFOLDED: ConvBN 3x3 -> ConvBN 3x3 -> Conv2d 1x1 (+bias) ->
    4 x 16 DFL logits per anchor -> DFL loss -> backward -> DDP gradient average -> optimiser step, over the trainer's three parameter groups
    (the unfolded counterpart of BoxBranchStep).  DetectBoxBranchStep(convs, w3, b3, ...) as _DetectBoxBranch takes them; `blocks`, `w3`, `b3`,
    `dw3`, `db3`, `cout3` are the branch's."""
    BRANCH = _DetectBoxBranch

    def forward_backward(self, x, target_ltrb, weight=None, target_scores_sum=1.0):
        """x bf16 [B,H,W,cin]; target_ltrb fp32 [B*H*W, 4] (bins), weight fp32 [B*H*W] or None -> (loss fp32[1], dx bf16 like x); every parameter
        gradient is left in the groups' gradient buffers."""
        out = self.branch.forward(x)
        loss, g = ops.dfl_loss(out.float().reshape(-1, self.cout3), target_ltrb, weight, target_scores_sum)
        return loss, self.branch.backward(g.reshape(out.shape).to(torch.bfloat16))


class DetectClassBranchStep(_BranchStep):
    """Ultralytics Detect.cv3[i] trained as the reference trains it (the counterpart of DetectBoxBranchStep): two `ClassBranchPair`s -> HeadOut(nc)
    -> BCE term of the OBB loss -> backward -> DDP gradient average -> optimiser step, over the trainer's three parameter groups.
    DetectClassBranchStep(pairs, w3, b3, ...) as _DetectClassBranch takes them; `pairs` and `out` are the branch's."""
    BRANCH = _DetectClassBranch

    def forward_backward(self, x, targets, target_scores_sum=1.0):
        """x bf16 [B,H,W,cin]; targets fp32 [B,H,W,nc] (or [B*H*W, nc]) -> (loss fp32[1], dx bf16 like x); every parameter gradient is left in the
        groups' gradient buffers."""
        logits = self.branch.forward(x)
        loss, g = ops.bce_loss(logits, targets.reshape(logits.shape), target_scores_sum)
        return loss, self.branch.backward(g)


def pad_targets(rows, B, imgsz, device=None):
    """The host-side `preprocess` of v8OBBLoss (Ultralytics 8.3.x, restated from recall: the package is not installed, so this is UNPINNED like
    `optimizer_config`): rows [n,7] = (batch_idx, cls, x, y, w, h, theta) with x, y, w, h normalised to the image -> (gt_labels int32 [B,n_max],
    gt_bboxes fp32 [B,n_max,5] in pixels, mask_gt bool [B,n_max]), each image's boxes first in their input order, zero rows behind them.  Boxes whose
    width or height is under 2 px are dropped.  imgsz = (H, W) or one int; n_max is at least 1, so an empty batch still has a (masked-out) row."""
    H, W = (imgsz, imgsz) if isinstance(imgsz, int) else imgsz
    r = torch.as_tensor(rows, dtype=torch.float32).reshape(-1, 7).cpu()
    px = r[:, 2:6] * torch.tensor([W, H, W, H], dtype=torch.float32)
    keep = (px[:, 2] >= 2) & (px[:, 3] >= 2)
    r, px = r[keep], px[keep]
    idx = r[:, 0].long()
    counts = torch.bincount(idx, minlength=B) if r.shape[0] else torch.zeros(B, dtype=torch.long)
    if counts.shape[0] > B:
        raise ValueError(f"pad_targets: batch index {int(idx.max())} with B = {B}")
    n_max = max(int(counts.max()), 1)
    gl = torch.zeros((B, n_max), dtype=torch.int32)
    gb = torch.zeros((B, n_max, 5), dtype=torch.float32)
    mk = torch.zeros((B, n_max), dtype=torch.bool)
    for j in range(B):
        sel = idx == j
        n = int(sel.sum())
        gl[j, :n] = r[sel, 1].to(torch.int32)
        gb[j, :n, :4] = px[sel]
        gb[j, :n, 4] = r[sel, 6]
        mk[j, :n] = True
    if device is not None:
        gl, gb, mk = gl.to(device), gb.to(device), mk.to(device)
    return gl, gb, mk


class OBBCriterion:
    """v8OBBLoss.__call__ on the head's own outputs (Ultralytics 8.3.x, restated from recall: UNPINNED, like `optimizer_config`; pinned by the tests against this
    repository's fp64 decode, loss terms and anchor grid): ops.crit_decode -> ops.rotated_tal_assign
    (topk 10, alpha 0.5, beta 6) -> ops.crit_loss.  __call__(box, cls, angle, gt_labels, gt_bboxes, mask_gt) with box / cls / angle the lists of the
    three levels' logits and the padded ground truth of `pad_targets` (on the device) -> (items fp32[3] = (box, cls, dfl) losses times their gains,
    (d_box, d_cls, d_angle)): the gradients of batch_size * sum(items) in the logits' layouts.  Everything stays on the device and on the current
    stream: no host read, so a whole call can be captured in a graph.  `last` keeps the assignment and tss of the latest call."""

    def __init__(self, nc, gains=(7.5, 0.5, 1.5), topk=10, alpha=0.5, beta=6.0):
        if not 1 <= nc <= 64:
            raise ValueError(f"OBBCriterion: nc = {nc}: 1..64")
        self.nc, self.gains, self.topk, self.alpha, self.beta = int(nc), tuple(float(g) for g in gains), topk, alpha, beta
        self.last = None

    def __call__(self, box, cls, angle, gt_labels, gt_bboxes, mask_gt):
        if cls[0].shape[-1] != self.nc:
            raise ValueError(f"OBBCriterion: class logits have {cls[0].shape[-1]} channels, nc = {self.nc}")
        pd_scores, pd_bboxes, anc_points, _ = ops.crit_decode(box, cls, angle)
        tl, tb, ts, fg, ti = ops.rotated_tal_assign(pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt, self.topk, self.alpha, self.beta)
        items, tss, d_box, d_cls, d_angle = ops.crit_loss(box, cls, angle, tb, ts, fg, self.gains)
        self.last = {"target_labels": tl, "target_bboxes": tb, "target_scores": ts, "fg_mask": fg, "target_gt_idx": ti, "tss": tss}
        return items, (d_box, d_cls, d_angle)


class DetectHead(_Step, _Composite):
    """The three levels of Ultralytics `Detect` / `OBB` (model.23: cv2 box, cv3 class, cv4 angle branches on P3, P4, P5) in training mode over ONE
    `ParamGroups`, trained under `OBBCriterion`.  levels: three dicts {"box": (convs, w3, b3), "cls": (pairs, w3, b3), "angle": (convs, w3, b3)} with
    convs / pairs as DetectBoxBranchStep / DetectClassBranchStep / DetectAngleBranch take them; per level the parameters are registered in the order
    box, cls, angle.  forward(feats) -> (box, cls, angle) lists (bf16 [B,H,W,64], fp32 [B,H,W,nc], fp32 [B,H,W,1]); backward(d_box, d_cls, d_angle) ->
    one dx per level, the sum of the three branches' input gradients through ops.add_bf16 in the fixed order (box + class) + angle;
    step(feats, gt_labels, gt_bboxes, mask_gt) = forward, criterion, backward, DDP gradient average, optimiser step -> (items, dx list).
    groups=: the head as part of a larger net (`Net`) on the caller's ParamGroups, which the caller builds; the branches are then registered in
    checkpoint order (all box branches, all class branches, all angle branches).
    `taps`: set `record_taps = True` and the next forward fills taps = {"in": feats, "out": (box, cls, angle)}; the next backward adds "dout" =
    (d_box, d_cls, d_angle), "branch_din" = [(dx_box, dx_cls, dx_angle)] per level, "partial" = [bf16(dx_box + dx_cls)] per level and "din" = the
    three sums it returns.  With the flag off nothing is kept (taps is None)."""

    def __init__(self, levels, nc, gains=(7.5, 0.5, 1.5), optimizer="SGD", lr=0.01, momentum=0.9, weight_decay=5e-4, nesterov=True, eps=1e-3,
                 bn_momentum=0.03, groups=None):
        if len(levels) != 3:
            raise ValueError("DetectHead: three levels (P3, P4, P5)")
        own = groups is None
        self.groups = ParamGroups(optimizer, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov) if own else groups
        self.box, self.cls, self.angle = [None] * 3, [None] * 3, [None] * 3
        fams = (("box", self.box, _DetectBoxBranch), ("cls", self.cls, _DetectClassBranch), ("angle", self.angle, DetectAngleBranch))
        # registration order: per level box, cls, angle on groups of its own; as part of a larger net (`Net`, the caller's groups, built by the
        # caller) CHECKPOINT order: cv2.0-2, cv3.0-2, cv4.0-2
        order = [(f, i) for i in range(3) for f in fams] if own else [(f, i) for f in fams for i in range(3)]
        for (key, dst, cls_), i in order:
            dst[i] = cls_(self.groups, *levels[i][key], eps, bn_momentum)
        for i in range(3):
            if self.box[i].cout3 != 64 or self.cls[i].out.c2 != nc or self.angle[i].out.c2 != 1:
                raise ValueError(f"DetectHead: a level's branches end in 64, nc = {nc} and 1 channels, got {self.box[i].cout3}, "
                                 f"{self.cls[i].out.c2}, {self.angle[i].out.c2}")
        if own:
            self.groups.build()
        self.criterion = OBBCriterion(nc, gains)
        self.record_taps, self.taps = False, None

    def children(self):
        """checkpoint order, whichever order the branches registered in"""
        return [(f"{cv}.{i}", b) for cv, fam in (("cv2", self.box), ("cv3", self.cls), ("cv4", self.angle)) for i, b in enumerate(fam)]

    def child_strides(self):
        """the input stride of every child: P3, P4, P5 per family"""
        return [8, 16, 32] * 3

    def forward(self, feats):
        out = ([b.forward(x) for b, x in zip(self.box, feats)], [c.forward(x) for c, x in zip(self.cls, feats)],
               [a.forward(x) for a, x in zip(self.angle, feats)])
        self.taps = {"in": list(feats), "out": out} if self.record_taps else None
        return out

    def backward(self, d_box, d_cls, d_angle):
        branch, partial, din = [], [], []
        for i in range(3):
            dxs = (self.box[i].backward(d_box[i]), self.cls[i].backward(d_cls[i]), self.angle[i].backward(d_angle[i]))
            p = ops.add_bf16(dxs[0], dxs[1])
            din.append(ops.add_bf16(p, dxs[2]))
            if self.record_taps:
                branch.append(dxs); partial.append(p)
        if self.record_taps:
            self.taps = dict(self.taps or {}, dout=(d_box, d_cls, d_angle), branch_din=branch, partial=partial, din=din)
        return din

    def forward_backward(self, feats, gt_labels, gt_bboxes, mask_gt):
        box, cls, angle = self.forward(feats)
        items, (d_box, d_cls, d_angle) = self.criterion(box, cls, angle, gt_labels, gt_bboxes, mask_gt)
        return items, self.backward(d_box, d_cls, d_angle)


class PackPlan:
    """This iteration's bf16 weights of MANY dense convs from one launch.  convs: layers with `_packed` (ConvBN, BoxOut) whose weights live in
    group 0 of `groups` (built); shapes: each layer's INPUT map (H, W).  The plan owns the device table (ops.conv_pack_plan) and ONE bf16 buffer
    with two segments per layer -- the forward form (stride-2 layers: the s2 layout) and the dgrad form -- and attaches itself to the layers
    (`layer.pack`), which then read views of that buffer in place of packing per call.  `run()` repacks everything from the flat group-0
    parameters (ops.conv_pack_multi_bf16: one launch, capturable); call it after every optimiser step and before the next forward (a layer that asks for its
    view after the flat parameters were written and before `run()` raises: stale weights are never read).  A layer asked
    for another H x W than planned raises: the layout depends on the map size.  `detach()` puts the layers back on per-call packing."""

    def __init__(self, groups, convs, shapes):
        convs, shapes = list(convs), [(int(h), int(w)) for h, w in shapes]
        if groups.opts is None or not convs or len(convs) != len(shapes):
            raise ValueError("PackPlan: built groups, and one (H, W) per layer of a non-empty list")
        self.flat = groups.opts[0].param
        layers = []
        for m, (H, W) in zip(convs, shapes):
            w = m.w
            if w.untyped_storage().data_ptr() != self.flat.untyped_storage().data_ptr() or not w.is_contiguous():
                raise ValueError("PackPlan: a layer's weights are no view of the groups' flat group-0 parameters")
            off = w.storage_offset() - self.flat.storage_offset()
            layers += [(m.c2, m.c1, m.k, m.s, H, W, f, off) for f in (0, 1)]
        self.table = ops.conv_pack_plan(self.flat.device, layers, self.flat.numel())
        self.packed = torch.zeros(self.table.total, dtype=torch.bfloat16, device=self.flat.device)
        seg = [self.packed[d:d + n] for d, n in zip(self.table.dst_off, self.table.n_elems)]
        self.convs, self._views, self._packed_version = convs, {}, None  # (None: never run)
        for i, (m, hw) in enumerate(zip(convs, shapes)):
            self._views[id(m)] = (hw, seg[2 * i], seg[2 * i + 1])
            m.pack = self

    def run(self):
        ops.conv_pack_multi_bf16(self.flat, self.table, out=self.packed)
        self._packed_version = self.flat._version

    def view(self, m, H, W, dgrad_form=False):
        hw, fwd, bwd = self._views[id(m)]
        if self.flat._version != self._packed_version:  # (torch counts the in-place writes of the flat parameters: an optimiser step, an EMA swap)
            raise RuntimeError("PackPlan: the parameters were written since the last run(): the packed weights are stale; call run() before the forward")
        if hw != (int(H), int(W)):
            raise ValueError(f"PackPlan: the layer {m.c1} -> {m.c2} was planned for {hw[0]} x {hw[1]} input maps and is asked for {H} x {W}: the packed layout "
                             "depends on the map size")
        return bwd if dgrad_form else fwd

    def detach(self):
        for m in self.convs:
            if m.pack is self:
                m.pack = None


def _state_block(params, name):
    """(w, gamma, beta, running_mean, running_var) of the Conv block `name` of an Ultralytics state dict (BatchNorm entries that are missing: None)"""
    return (params[name + ".conv.weight"],) + tuple(params.get(f"{name}.bn.{k}") for k in ("weight", "bias", "running_mean", "running_var"))


class Trunk(_Composite):
    """Models 0-22 of yolo11-obb.yaml (backbone + FPN / PAN neck) in training mode over ONE `ParamGroups` (the caller builds it after the
    constructor).  params: a dict keyed by Ultralytics state-dict names (`model.2.m.0.cv1.conv.weight`, `...bn.weight`, `...bn.bias`,
    `...bn.running_mean`, `...bn.running_var`); scale "n" or "s".  The parameters are registered in checkpoint order: model.0, model.1,
    model.2.cv1, model.2.cv2, model.2.m.0.cv1, ...

        0 stem  1 Conv s2  2 C3k2  3 Conv s2  4 C3k2  5 Conv s2  6 C3k2(c3k)  7 Conv s2  8 C3k2(c3k)  9 SPPF  10 C2PSA
        12 = cat(up(10), 6) -> 13 C3k2    15 = cat(up(13), 4) -> 16 C3k2 (P3)    17 Conv s2    18 = cat(17, 13) -> 19 C3k2 (P4)
        20 Conv s2    21 = cat(20, 10) -> 22 C3k2(c3k) (P5)

    forward(tiles uint8 [B,H,W,3|4], H and W multiples of 32) -> [P3, P4, P5] bf16 NHWC; backward([d3, d4, d5]) writes every parameter gradient.
    Six tensors have two consumers.  Each one's gradient is ops.add_bf16(first, second) = bf16(fp32 + fp32), FIRST the gradient of the consumer
    that comes LATER in the yaml (the one the backward reaches first), SECOND that of the earlier one:
        19: head P4 + model.20      16: head P3 + model.17      13: concat 18 + upsample/concat 15      10: concat 21 + upsample/concat 12
         6: concat 12 + model.7      4: concat 15 + model.5
    `taps`: set `record_taps = True` and the next forward / backward fill taps[i] = {"in", "out", "dout", "din"} per top-level module i (the
    concat modules under 12, 15, 18, 21 with "in" = (a, b), "din" = (da, db)) and taps["fan"][i] = (first, second, sum) per fan-out tensor."""

    SCALES = {"n": 16, "s": 32}  # stem width = make_divisible(64 * width, 8): the scales `train_kernel_of` and the shape catalogue cover
    IN_LEVEL = {0: 1, 1: 2, 2: 4, 3: 4, 4: 8, 5: 8, 6: 16, 7: 16, 8: 32, 9: 32, 10: 32, 13: 16, 16: 8, 17: 8, 19: 16, 20: 16, 22: 32}  # input stride per module that owns layers
    CONVS, C3K2S = (1, 3, 5, 7, 17, 20), (2, 4, 6, 8, 13, 16, 19, 22)

    def __init__(self, groups, params, scale="n", eps=1e-3, momentum=0.03):
        if scale not in self.SCALES:
            raise ValueError(f"Trunk: scale {scale!r}: the training kernels cover the n and s scales")
        t = lambda name: _state_block(params, name)
        if params["model.0.conv.weight"].shape[0] != self.SCALES[scale]:
            raise ValueError(f"Trunk: model.0 has {params['model.0.conv.weight'].shape[0]} channels, scale {scale!r} has {self.SCALES[scale]}")
        self.groups, self.scale, self.m = groups, scale, {}
        self.record_taps, self.taps = False, None

        def bneck(p):
            return (t(p + ".cv1"), t(p + ".cv2"))

        def c3k2(i):
            p, members, c3k = f"model.{i}", [], f"model.{i}.m.0.cv3.conv.weight" in params
            while f"{p}.m.{len(members)}.cv1.conv.weight" in params:
                q = f"{p}.m.{len(members)}"
                if c3k:
                    inner = []
                    while f"{q}.m.{len(inner)}.cv1.conv.weight" in params:
                        inner.append(bneck(f"{q}.m.{len(inner)}"))
                    members.append((t(q + ".cv1"), t(q + ".cv2"), t(q + ".cv3"), inner))
                else:
                    members.append(bneck(q))
            return C3k2(groups, t(p + ".cv1"), t(p + ".cv2"), members, c3k=c3k, eps=eps, momentum=momentum)

        for i in range(23):
            if i == 0:
                self.m[0] = _bn_block(StemConvBN, groups, t("model.0"), eps, momentum)
            elif i in self.CONVS:
                self.m[i] = _bn_block(ConvBN, groups, t(f"model.{i}"), eps, momentum, s=2)
            elif i in self.C3K2S:
                self.m[i] = c3k2(i)
            elif i == 9:
                self.m[9] = SPPF(groups, t("model.9.cv1"), t("model.9.cv2"), eps, momentum)
            elif i == 10:
                blocks = []
                while f"model.10.m.{len(blocks)}.attn.qkv.conv.weight" in params:
                    q = f"model.10.m.{len(blocks)}"
                    blocks.append(tuple(t(f"{q}.{n}") for n in PSABlock.NAMES))
                nh = params["model.10.cv1.conv.weight"].shape[0] // 128
                self.m[10] = C2PSA(groups, t("model.10.cv1"), t("model.10.cv2"), blocks, nh, eps, momentum)
            elif i in (12, 15):
                self.m[i] = UpCat(2)
            elif i in (18, 21):
                self.m[i] = UpCat(1)
        self.ch = self.m[0].c1

    def children(self):
        """the modules that own layers under their state-dict names, checkpoint = registration order (the concat modules own none)"""
        return [(f"model.{i}", self.m[i]) for i in sorted(self.IN_LEVEL)]

    def child_strides(self):
        """the input stride of every child"""
        return [self.IN_LEVEL[i] for i in sorted(self.IN_LEVEL)]

    def _f(self, i, *xs):
        y = self.m[i].forward(*xs)
        if self.taps is not None:
            self.taps[i] = {"in": xs[0] if len(xs) == 1 else xs, "out": y}
        return y

    def _b(self, i, d):
        r = self.m[i].backward(d)
        if self.taps is not None:
            self.taps[i].update(dout=d, din=r)
        return r

    def _sum(self, i, first, second):
        s = ops.add_bf16(first, second)
        if self.taps is not None:
            self.taps["fan"][i] = (first, second, s)
        return s

    def forward(self, tiles):
        if tiles.dim() != 4 or tiles.shape[1] % 32 or tiles.shape[2] % 32 or tiles.shape[3] != self.ch:
            raise ValueError(f"Trunk.forward: tiles uint8 [B,H,W,{self.ch}] with H and W multiples of 32, got {tuple(tiles.shape)}")
        self.taps = {"fan": {}} if self.record_taps else None
        x = tiles
        keep = {}
        for i in range(11):
            x = keep[i] = self._f(i, x)
        x13 = self._f(13, self._f(12, keep[10], keep[6]))
        x16 = self._f(16, self._f(15, x13, keep[4]))
        x19 = self._f(19, self._f(18, self._f(17, x16), x13))
        x22 = self._f(22, self._f(21, self._f(20, x19), keep[10]))
        return [x16, x19, x22]

    def backward(self, d):
        d3, d4, d5 = d
        d20, d10a = self._b(21, self._b(22, d5))
        g19 = self._sum(19, d4, self._b(20, d20))
        d17, d13a = self._b(18, self._b(19, g19))
        g16 = self._sum(16, d3, self._b(17, d17))
        d13b, d4a = self._b(15, self._b(16, g16))
        d10b, d6a = self._b(12, self._b(13, self._sum(13, d13a, d13b)))
        g = self._sum(10, d10a, d10b)
        for i in (10, 9, 8):
            g = self._b(i, g)
        g = self._sum(6, d6a, self._b(7, g))
        g = self._sum(4, d4a, self._b(5, self._b(6, g)))
        for i in (4, 3, 2, 1, 0):
            g = self._b(i, g)


class Net(_Step, _Composite):
    """The whole YOLO11-OBB training iteration: `Trunk` (models 0-22) + the branches of `DetectHead` (model.23) + `OBBCriterion` over ONE
    `ParamGroups`, the parameters registered in checkpoint order (the trunk's, then model.23.cv2.0-2, cv3.0-2, cv4.0-2).  params: a dict keyed by
    Ultralytics state-dict names (`Trunk`; the head's plain convs as `model.23.cv2.0.2.weight` / `.bias`); scale "n" or "s" (anything else:
    ValueError); ch = 3 or 4.
        forward_backward(tiles uint8 [B,H,W,ch], gt_labels, gt_bboxes, mask_gt) -> items fp32[3] (the ground truth of `pad_targets`, on the device)
        step(..., ni=, epoch=) with `net.update = TrainerUpdate(net.groups, ...)`, or step(...) for the plain optimiser step (`_Step`)
    The dense convs' bf16 weights come from ONE launch per iteration (`PackPlan`, built lazily for the tile size seen, run first thing in
    forward_backward); `pack = False` packs per layer and call as the blocks do on their own -- the results are bit-identical.  `taps`: set
    `record_taps = True`; the next forward_backward fills taps[0..22] and taps["fan"] (`Trunk`) and taps[23] = {"in": [P3, P4, P5], "out": (box, cls,
    angle), "dout": (d_box, d_cls, d_angle), "din": [d3, d4, d5]} plus the head's own "branch_din" and "partial" (`DetectHead`: the three summands of
    every d and the sum of the first two)."""

    def __init__(self, params, scale="n", nc=12, ch=3, gains=(7.5, 0.5, 1.5), optimizer="SGD", lr=0.01, momentum=0.9, weight_decay=5e-4, nesterov=True,
                 eps=1e-3, bn_momentum=0.03, pack=True):
        w0 = params["model.0.conv.weight"]
        if w0.shape[1] != ch:
            raise ValueError(f"Net: model.0 reads {w0.shape[1]} channels, ch = {ch}")
        self.groups = ParamGroups(optimizer, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov)
        self.trunk = Trunk(self.groups, params, scale, eps, bn_momentum)
        t = lambda name: _state_block(params, name)
        wb = lambda name: (params[name + ".weight"], params[name + ".bias"])
        levels = []
        for i in range(3):
            b, c, a = f"model.23.cv2.{i}", f"model.23.cv3.{i}", f"model.23.cv4.{i}"
            levels.append({"box": ([t(b + ".0"), t(b + ".1")], *wb(b + ".2")),
                           "cls": ([(t(c + ".0.0"), t(c + ".0.1")), (t(c + ".1.0"), t(c + ".1.1"))], *wb(c + ".2")),
                           "angle": ([t(a + ".0"), t(a + ".1")], *wb(a + ".2"))})
        self.head = DetectHead(levels, nc, gains, eps=eps, bn_momentum=bn_momentum, groups=self.groups)
        self.groups.build()
        self.scale, self.nc, self.ch, self.pack = scale, int(nc), int(ch), bool(pack)
        self.plan, self._plan_hw = None, None
        self.record_taps, self.taps = False, None

    @classmethod
    def from_state(cls, params, scale="n", nc=12, ch=3, **kw):
        return cls(params, scale, nc, ch, **kw)

    criterion = property(lambda self: self.head.criterion)

    def children(self):
        """the trunk's modules, then the head's branches as model.23.*: named_blocks() lists every layer under its state-dict name in registration
        order, fold() every conv of the model (the head's plain output convs as they are)"""
        return self.trunk.children() + [(f"model.23.{n}", b) for n, b in self.head.children()]

    def pack_layers(self, H, W):
        """[(layer, (h, w))] for a `PackPlan`: every leaf with `_packed` and its input map at H x W tiles -- the stride is its top-level module's"""
        strides = self.trunk.child_strides() + self.head.child_strides()
        return [(b, (H // lv, W // lv)) for (name, m), lv in zip(self.children(), strides) for _, b in _flatten(name, m) if hasattr(b, "_packed")]

    validator = None

    def validate(self, pool, **kw):
        """One validation of this net on `pool` (a `TrainBatcher`, or its three pool tensors) -> `Validator`'s result dict.  The `Validator` is kept
        (`self.validator`, with its `best_fitness` / `is_best`) and reused while `pool` is the same object and the keyword arguments are equal.
        Another pool or other arguments make a NEW one: the old one is closed (its engine slot released at once) and `best_fitness` starts over --
        hold a `Validator` of your own where the best fitness has to outlive such a change."""
        v = self.validator
        if v is None or v.made_from[0] is not pool or v.made_from[1] != kw:
            if v is not None:
                v.close()
            v = self.validator = Validator(self, pool, **kw)
            v.made_from = (pool, dict(kw))
        return v()

    def _attach(self, H, W):
        if not self.pack:
            return
        if self._plan_hw != (H, W):
            if self.plan is not None:
                self.plan.detach()
            self.plan, self._plan_hw = PackPlan(self.groups, *zip(*self.pack_layers(H, W))), (H, W)
        self.plan.run()

    def forward_backward(self, tiles, gt_labels, gt_bboxes, mask_gt):
        self._attach(tiles.shape[1], tiles.shape[2])
        self.trunk.record_taps = self.head.record_taps = self.record_taps
        feats = self.trunk.forward(tiles)
        box, cls, angle = self.head.forward(feats)
        items, dlog = self.criterion(box, cls, angle, gt_labels, gt_bboxes, mask_gt)
        dfe = self.head.backward(*dlog)
        self.trunk.backward(dfe)
        self.taps = self.trunk.taps
        if self.taps is not None:
            h = self.head.taps
            self.taps[23] = {"in": feats, "out": (box, cls, angle), "dout": dlog, "din": dfe, "branch_din": h["branch_din"], "partial": h["partial"]}
        return items


def clip_grad_norm(groups_or_flat_grads, max_norm=10.0):
    """`torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=10.0)` of the trainer's optimizer_step over the flat gradient buffers (a
    ParamGroups, or a list of flat fp32 tensors) in two launches -> clip fp32[3] ON THE DEVICE = (total_norm, coef, finite).  The gradients are
    not scaled here: `ParamGroups.step(..., clip=clip)` multiplies by coef as it reads them.  Nothing is read back to the host."""
    g = groups_or_flat_grads
    return ops.clip_grad_norm(g.flat_grads() if hasattr(g, "flat_grads") else list(g), max_norm)


class Schedule:
    """The trainer's per-iteration learning rate, momentum and accumulation count (Ultralytics 8.3.x `BaseTrainer._setup_scheduler` and the
    warm-up block of `_do_train`, restated from recall: the package is not installed, so this is UNPINNED like `optimizer_config`).  Host only,
    in double.  nb = batches per epoch; ni = the global iteration (epoch * nb + batch index).
        nw = max(round(warmup_epochs * nb), 100) warm-up iterations;  lf(x) = max(1 - x / epochs, 0) (1 - lrf) + lrf  (linear), or
        lf(x) = lrf + (1 - lrf) (1 + cos(x pi / epochs)) / 2  (cos_lr; the trainer's ((1 - cos(x pi / epochs)) / 2) (lrf - 1) + 1 written so
        that both end points are exact: lf(0) = 1, lf(epochs) = lrf);
        ni <= nw:  lr = interp(ni, [0, nw], [warmup_bias_lr for the bias group else 0, lr0 lf(epoch)]), momentum = interp(ni, [0, nw],
                   [warmup_momentum, momentum]), accumulate = max(1, round(interp(ni, [0, nw], [1, nbs / batch])));
        after:     lr = lr0 lf(epoch) for every group, `momentum`, accumulate = max(1, round(nbs / batch)).
    `at(ni, epoch)` -> {"lr": (weights, norm weights, biases) in ParamGroups' group order, "momentum", "accumulate"}; for AdamW the scheduled
    momentum is betas[0] (`ParamGroups.step(momentum=)`).  Train_OBB.py:792-841 trains with lr0 = 0.003, lrf = 0.05."""

    def __init__(self, epochs, nb, lr0, lrf=0.01, momentum=0.937, cos_lr=False, warmup_epochs=3.0, warmup_momentum=0.8, warmup_bias_lr=0.1, batch=16,
                 nbs=64):
        if epochs < 1 or nb < 1 or batch < 1:
            raise ValueError("Schedule: epochs, nb and batch are at least 1")
        self.epochs, self.nb, self.lr0, self.lrf, self.momentum, self.cos_lr = int(epochs), int(nb), float(lr0), float(lrf), float(momentum), bool(cos_lr)
        self.warmup_momentum, self.warmup_bias_lr, self.batch, self.nbs = float(warmup_momentum), float(warmup_bias_lr), int(batch), int(nbs)
        self.nw = max(round(warmup_epochs * nb), 100)

    def lf(self, x):
        if self.cos_lr:
            return self.lrf + (1.0 - self.lrf) * ((1.0 + math.cos(x * math.pi / self.epochs)) / 2.0)
        return max(1.0 - x / self.epochs, 0.0) * (1.0 - self.lrf) + self.lrf

    def at(self, ni, epoch):
        import numpy as np
        base = self.lr0 * self.lf(epoch)
        full = self.nbs / self.batch
        if ni > self.nw:
            return {"lr": (base, base, base), "momentum": self.momentum, "accumulate": max(1, round(full))}
        xi = [0, self.nw]
        lr = float(np.interp(ni, xi, [0.0, base]))
        return {"lr": (lr, lr, float(np.interp(ni, xi, [self.warmup_bias_lr, base]))),
                "momentum": float(np.interp(ni, xi, [self.warmup_momentum, self.momentum])),
                "accumulate": max(1, round(float(np.interp(ni, xi, [1, full]))))}


class ModelEMA:
    """Ultralytics `ModelEMA(model, decay=0.9999, tau=2000)` over a built ParamGroups: flat copies of the three parameter buffers AND of `buffers`
    (the BatchNorm running statistics: the trainer's EMA runs over the whole float state dict), averaged by ONE launch per `update()`
    (ops.ema_update) with d = decay (1 - exp(-updates / tau)).  The EMA model is the one the trainer validates and saves: `with ema.applied():`
    puts its values into the groups (and takes them out again), so every block's `fold()` inside the context is the EMA model's."""

    def __init__(self, groups, decay=0.9999, tau=2000):
        if groups.opts is None:
            raise RuntimeError("ModelEMA: groups.build() first")
        self.groups, self.decay, self.tau, self.updates = groups, float(decay), float(tau), 0
        self.ema = [t.clone() for t in self.live()]

    def live(self):
        """the four flat buffers the EMA follows"""
        return [o.param for o in self.groups.opts] + [self.groups.buffers]

    def decay_at(self, updates):
        return self.decay * (1.0 - math.exp(-updates / self.tau))

    def update(self):
        self.updates += 1
        ops.ema_update(self.ema, self.live(), self.decay_at(self.updates))

    def applied(self):
        import contextlib

        @contextlib.contextmanager
        def swap():
            live = self.live()
            scratch = [t.clone() for t in live]
            for t, e in zip(live, self.ema):
                t.copy_(e)
            try:
                yield self
            finally:
                for t, s in zip(live, scratch):
                    t.copy_(s)
        return swap()


class TrainerUpdate:
    """Everything the trainer does between `loss.backward()` and the next forward (Ultralytics 8.3.x `_do_train` / `optimizer_step`, restated from
    recall, UNPINNED like `Schedule`), on a built ParamGroups whose gradient buffers the backward has just written:
        the schedule's lr / momentum / accumulate at (ni, epoch);  accumulate > 1: the gradients are added into accumulation buffers;
        when ni - last_opt_step >= accumulate:  DDP gradient average of the buffers being stepped -> `clip_grad_norm` (max_norm 10) ->
        `groups.step(lr, momentum, clip)` -> `ema.update()`.
    __call__(ni, epoch, group=None) -> the clip tensor (fp32[3] on the device) at an optimiser step, None between two.  A fixed number of launches
    per update whatever the number of layers (accumulate 1, sumsq 1, coefficient 1, step 1, EMA 1), and no host read.  `last_opt_step` starts at -1
    as the trainer's; set it when resuming."""

    def __init__(self, groups, schedule, max_norm=10.0, ema=None):
        if groups.opts is None:
            raise RuntimeError("TrainerUpdate: groups.build() first")
        self.groups, self.schedule, self.max_norm, self.ema = groups, schedule, float(max_norm), ema
        self.last_opt_step, self.acc, self.n_acc = -1, None, 0

    def __call__(self, ni, epoch, group=None):
        s = self.schedule.at(ni, epoch)
        grads = [o.grad for o in self.groups.opts]
        if s["accumulate"] > 1 or self.n_acc:
            if self.acc is None:
                self.acc = [torch.empty_like(g) for g in grads]
            ops.grad_accumulate(self.acc, grads, first=self.n_acc == 0)
            self.n_acc += 1
            grads = self.acc
        if ni - self.last_opt_step < s["accumulate"]:
            return None
        allreduce_gradients([g for g in grads if g.numel()], group)
        clip = clip_grad_norm(grads, self.max_norm)
        self.groups.step(s["lr"], s["momentum"], clip, grads=grads)
        if self.ema is not None:
            self.ema.update()
        self.last_opt_step, self.n_acc = ni, 0
        return clip


# yolo11-obb.yaml `scales`: depth, width, max_channels of the scales `Trunk` trains (the blob's header carries them)
_YAML_SCALES = {"n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024)}
_REG_MAX = 16


class FoldPlan:
    """The "OBBW" weight blob of a built `Net` (the format `obb_model_load` parses: header, record table, fp32 data section), refreshed from the
    flat parameter buffers by ONE launch and ONE device-to-host copy.  The constructor writes the header and the record table once, on the host --
    record names from `Net.named_blocks()` (the trunk's, then the head's, checkpoint order), c1 / c2 / k / s / g / act from the blocks -- into a
    buffer that is pinned when the net lives on a device, and builds the kernel's table (ops.fold_blob_plan).  `run(ema=None)` folds the live
    buffers, or `ema.ema` (a `ModelEMA`'s copies: no `ema.applied()` swap, nothing of the net is written), into the data section and returns the
    whole blob as a memoryview of that buffer, valid until the next `run()`.  The arithmetic is `_BNBlock.fold()`'s in IEEE fp32: a leaf without
    BatchNorm is copied, one with `order` set (the qkv convs; the kernel knows that one permutation) comes back in checkpoint order.  On a CPU-built net the header and table are there (`blob`), `run()` raises: there is no CPU path."""

    def __init__(self, net):
        import numpy as np
        from . import _lib
        groups = net.groups
        if groups.opts is None:
            raise RuntimeError("FoldPlan: the net's groups are not built")
        if net.scale not in _YAML_SCALES:
            raise ValueError(f"FoldPlan: scale {net.scale!r}")
        self.net, self.flats = net, [o.param for o in groups.opts] + [groups.buffers]

        def off(t, k):
            flat = self.flats[k]
            if t.untyped_storage().data_ptr() != flat.untyped_storage().data_ptr() or not t.is_contiguous():
                raise ValueError("FoldPlan: a layer's tensor is no view of the groups' flat buffers")
            return t.storage_offset() - flat.storage_offset()

        blocks = net.named_blocks()
        eps = {b.eps for _, b in blocks if hasattr(b, "gamma")}
        if len(eps) != 1:
            raise ValueError(f"FoldPlan: the BatchNorm blocks carry different eps {sorted(eps)}: one launch folds with one")
        self.eps = eps.pop()
        depth, width, max_ch = _YAML_SCALES[net.scale]
        hdr = struct.pack("<4sIIiiffii", b"OBBW", 1, len(blocks), net.nc, net.ch, width, depth, max_ch, _REG_MAX) + struct.pack("<8s", net.scale.encode())
        rec_size = 64 + 6 * 4 + 2 * 8
        self.data_off = (len(hdr) + rec_size * len(blocks) + 63) // 64 * 64
        table, recs, o = b"", [], self.data_off
        self.names = [name for name, _ in blocks]
        for name, b in blocks:
            if len(name.encode()) > 63:
                raise ValueError(f"FoldPlan: record name too long: {name}")
            per = (b.c1 // b.g) * b.k * b.k
            if tuple(b.w.shape) != (b.c2, b.c1 // b.g, b.k, b.k):
                raise ValueError(f"FoldPlan: {name}: weights {tuple(b.w.shape)}")
            table += struct.pack("<64siiiiiiQQ", name.encode(), b.c1, b.c2, b.k, b.s, b.g, int(b.act), o, o + 4 * b.c2 * per)
            o += 4 * b.c2 * (per + 1)
            if not hasattr(b, "gamma"):  # no BatchNorm: a plain conv with bias
                recs.append((_lib.FOLD_PLAIN, off(b.w, 0), 0, off(b.b, 2), 0, 0, b.c2, per))
                continue
            if b.order is not None and not torch.equal(b.order.cpu(), torch.argsort(qkv_device_order(b.c2 // 128))):
                raise ValueError(f"FoldPlan: {name}: the fold kernel knows one row order, the inverse of qkv_device_order({b.c2 // 128})")
            kind = _lib.FOLD_BN if b.order is None else _lib.FOLD_QKV
            recs.append((kind, off(b.w, 0), off(b.gamma, 1), off(b.beta, 2), off(b.running_mean, 3), off(b.running_var, 3), b.c2, per))
        self.nbytes = o
        dev = self.flats[0].device
        self._buf = torch.zeros(o, dtype=torch.uint8, pin_memory=dev.type == "cuda")
        self._np = self._buf.numpy()
        head = hdr + table
        self._np[:self.data_off] = np.frombuffer(head + b"\0" * (self.data_off - len(head)), np.uint8)
        self._data = self._buf[self.data_off:].view(torch.float32)
        self.records = recs
        self.table = ops.fold_blob_plan(dev, recs) if dev.type == "cuda" else None
        self.host_table = ops.fold_blob_table(recs)
        if 4 * int(self.host_table[2]) != o - self.data_off:
            raise RuntimeError("FoldPlan: the kernel table and the blob's record table disagree about the data section")
        self.out = torch.empty(int(self.host_table[2]), dtype=torch.float32, device=dev) if dev.type == "cuda" else None

    @property
    def blob(self):
        """the whole blob (header, table, data section as of the last `run()`) as a memoryview of the plan's host buffer"""
        return memoryview(self._np)

    def fold(self, ema=None):
        """the launch alone -> the data section on the device (fp32, `self.out`)"""
        if self.table is None:
            raise RuntimeError("FoldPlan: the net is on the CPU; the fold is a HIP kernel and has no CPU path")
        srcs = self.flats if ema is None else ema.ema
        if len(srcs) != 4 or any(a.shape != b.shape for a, b in zip(srcs, self.flats)):
            raise ValueError("FoldPlan: `ema` is no ModelEMA over this net's groups")
        return ops.fold_blob_f32(*srcs, self.table, self.eps, out=self.out)

    def run(self, ema=None):
        self._data.copy_(self.fold(ema), non_blocking=True)
        torch.cuda.current_stream(self.out.device).synchronize()
        return self.blob


class Validator:
    """The trainer's validation of the net being trained (Ultralytics 8.3.x `OBBValidator` behind `model.train(...)`, Train_OBB.py:792-841; restated
    from recall: the package is not installed, so conf 0.001, iou 0.7, max_det 300, the matching rule, the 101-point AP and fitness = 0.1 mAP50 +
    0.9 mAP50-95 are UNPINNED, like `Schedule` and `optimizer_config`).  Validator(net, pool, ...)() does, in order:
        FoldPlan.run(ema)  ->  model.YOLO.reload(blob) into an engine slot of the validator's own  ->  per batch of `batch` pool tiles, in pool
        order: the tiles and their `xywhr` targets from ops.aug_tiles / ops.aug_labels under IDENTITY records (no mosaic, affine, HSV or flip),
        `YOLO.predict_tiles`, ops.val_match  ->  ONE read-back of confidences, classes, true-positive bits and target classes  ->
        metrics.ap_per_class
    and returns {"map50", "map", "fitness", "ap" [classes present, 10], "n_det", "n_gt"}; `best_fitness` / `is_best` follow the calls (is_best:
    this call's fitness is at least every earlier one's, the trainer's rule for `best.pt`).  pool: a `TrainBatcher` or its three pool tensors
    (tiles uint8 [N,s,s,C], labels fp64 [N,Lmax,9], counts int32 [N]); the tiles go to the engine as stored -- BGR, what `YOLO` expects -- unless
    `swap_rb`.  ema: a `ModelEMA` over the net's groups (the model the trainer validates) or None for the live parameters.  Nothing of the net,
    its optimiser state or the EMA is written, and the engine context's active slot and options are left as found (ops.engine_state).
    `update(det, count, gt_labels, gt_bboxes, mask_gt)` adds given detections to the statistics and `result()` cumulates them: matching and AP
    can be driven without the net's forward (`reset()` first).  `close()` releases the engine slot.
    Targets: the label kernel runs with NEUTRAL candidate thresholds (no minimum side, aspect or area ratio: the training filter of
    `AugmentConfig` is not applied), so every label of the pool counts, with two exceptions that are the trainer's own -- a label whose rectangle
    clipped to the tile has a side under 2 px is dropped (`pad_targets`' rule, inside ops.aug_labels), and a tile with more than `n_cap` labels
    raises ValueError at the read-back rather than losing ground truth silently.
    report=True adds the rest of the trainer's per-epoch row (UNPINNED like the above).  Per batch, on the device and without a host read: the
    training loss of the engine's own head rows -- ops.val_crit_decode -> ops.rotated_tal_assign (the net's `OBBCriterion` topk / alpha / beta) ->
    ops.val_crit_items, ACCUMULATED into one items buffer -- and ops.val_confusion (detections above `cm_conf`, class-agnostic ProbIoU above
    `cm_iou`) into one matrix.  Both come back with `result()`'s read-back, and `report()` then returns the six keys of `__call__` plus
    {"box_loss", "cls_loss", "dfl_loss" (accumulated item / number of batches: the trainer's rule), "precision", "recall" (`mp` / `mr` of
    metrics.pr_curves), "f1" (the class mean at that point), "conf_best", "curves" (pr_curves' whole dict), "confusion" int64 [nc+1, nc+1]:
    [predicted, true], the last row / column = background}.  `__call__`'s return value and `best_fitness` / `is_best` do not change with the flag.
    `update(..., head=None)` without head rows counts the confusion matrix and no loss batch."""

    def __init__(self, net, pool, batch=16, conf=0.001, iou=0.7, max_det=300, precision="f32", ema=None, n_cap=64, swap_rb=False, report=False,
                 cm_conf=0.25, cm_iou=0.45):
        from .augment import TrainBatcher
        if isinstance(pool, TrainBatcher):
            pool = (pool.tiles, pool.labels, pool.counts)
        from .augment import AugmentConfig
        neutral = AugmentConfig(wh_thr=-1.0, ar_thr=float("inf"), area_thr=-1.0)  # box_candidates keeps everything: validation drops no target
        self.batcher = TrainBatcher(*pool, cfg=neutral, n_cap=n_cap, bgr=True, swap_rb=swap_rb)
        if self.batcher.tiles.shape[3] != net.ch or self.batcher.s % 32:
            raise ValueError(f"Validator: the net reads {net.ch}-channel tiles with a side that is a multiple of 32, the pool holds "
                             f"{tuple(self.batcher.tiles.shape[1:])}")
        if batch < 1 or max_det < 1:
            raise ValueError("Validator: batch and max_det are at least 1")
        self.net, self.ema, self.batch, self.conf, self.iou, self.max_det, self.precision = net, ema, int(batch), float(conf), float(iou), int(max_det), precision
        self.plan = FoldPlan(net)
        self.device = self.batcher.tiles.device
        self.model, self.thr = None, ops.val_thresholds(self.device)
        self.table = self._identity_table()
        self.bufs = self.batcher.buffers(min(self.batch, self.batcher.N))
        self.tiles = None  # the tiles of the latest batch as the engine read them
        self.best_fitness, self.is_best, self.last = None, False, None
        self.report_on, self.cm_conf, self.cm_iou = bool(report), float(cm_conf), float(cm_iou)
        if self.report_on:
            self.loss_items = torch.zeros(3, dtype=torch.float32, device=self.device)
            self.loss_tss = torch.zeros(1, dtype=torch.float32, device=self.device)
            self.confusion = torch.zeros((net.nc + 1, net.nc + 1), dtype=torch.int32, device=self.device)
        self.reset()

    def _identity_table(self):
        import numpy as np
        from . import augment
        t = np.zeros(self.batcher.N, augment.REC)
        for i in range(self.batcher.N):
            augment.make_record(t[i], np.eye(3), 1.0, self.batcher.s, src=(i, 0, 0, 0))
        augment.check_table(t, self.batcher.N, self.batcher.s)
        return augment.table_to_device(t, self.device)

    def reset(self):
        self.stats, self._label_counts = [], []
        self._loss_batches, self._report = 0, None
        if self.report_on:
            self.loss_items.zero_()
            self.confusion.zero_()

    def close(self):
        """releases the validator's engine slot (weights, plans, slabs); the next call loads a model again"""
        if self.model is not None:
            self.model.close()
            self.model = None

    def update(self, det, count, gt_labels, gt_bboxes, mask_gt, head=None):
        """det [B,max_det,7] / count [B] as `YOLO.predict_tiles` returns them, the padded targets in pixels (device) -> (tp, best_iou, best_gt) of
        ops.val_match; the batch joins the statistics `result()` cumulates (device tensors: nothing is read back here).  With report=True the
        batch also joins the confusion matrix and, given `head` (the raw head rows of `predict_tiles(..., return_head=True)`), the loss items."""
        tp, bi, bg = ops.val_match(det, count, gt_labels, gt_bboxes, mask_gt, self.net.nc, self.thr)
        self.stats.append((tp, det[:, :, 4:6].contiguous(), count.clone(), gt_labels.clone(), mask_gt.clone()))
        if self.report_on:
            ops.val_confusion(det, count, gt_labels, gt_bboxes, mask_gt, self.net.nc, self.cm_conf, self.cm_iou, matrix=self.confusion)
            if head is not None:
                c, s = self.net.criterion, self.batcher.s
                ps, pb, ap, _ = ops.val_crit_decode(head, s, s, self.net.nc)
                _, tb, ts, fg, _ = ops.rotated_tal_assign(ps, pb, ap, gt_labels, gt_bboxes, mask_gt, c.topk, c.alpha, c.beta)
                ops.val_crit_items(head, s, s, self.net.nc, tb, ts, fg, c.gains, items=self.loss_items, tss=self.loss_tss, accumulate=True)
                self._loss_batches += 1
        return tp, bi, bg

    def result(self):
        """the statistics since `reset()` -> {"map50", "map", "fitness", "ap", "n_det", "n_gt"} (the one read-back, then numpy float64)"""
        import numpy as np
        from . import metrics
        nt = self.thr.numel()
        if self.stats:
            tp, cc, cnt, gl, mk = (torch.cat(ts).cpu() for ts in zip(*self.stats))
            live = (torch.arange(tp.shape[1])[None, :] < cnt.clamp(0, tp.shape[1])[:, None]).numpy()
            bits = tp.numpy()[live]
            tpb = ((bits[:, None].astype(np.int64) >> np.arange(nt)[None, :]) & 1).astype(bool)
            conf, cls = cc[..., 0].numpy()[live], cc[..., 1].numpy()[live]
            target = gl.numpy()[mk.numpy().astype(bool)]
            if self._label_counts and int(torch.cat(self._label_counts).max()) > self.batcher.n_cap:  # (read back with the rest)
                raise ValueError(f"Validator: a tile has {int(torch.cat(self._label_counts).max())} labels, n_cap = {self.batcher.n_cap}: ground truth would be lost; "
                                 "raise n_cap (at most 512)")
        else:
            tpb, conf, cls, target = np.zeros((0, nt), bool), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32)
        r = metrics.ap_per_class(tpb, conf, cls, target, self.net.nc)
        out = {"map50": r["map50"], "map": r["map"], "fitness": r["fitness"], "ap": r["ap"], "n_det": int(len(conf)), "n_gt": int(len(target))}
        if self.report_on:
            items = self.loss_items.cpu().numpy().astype(np.float64) / max(self._loss_batches, 1)  # (with the read-back above)
            c = metrics.pr_curves(tpb, conf, cls, target, self.net.nc)
            self._report = dict(out, box_loss=float(items[0]), cls_loss=float(items[1]), dfl_loss=float(items[2]), precision=c["mp"], recall=c["mr"],
                                f1=float(c["f1"].mean()) if len(c["f1"]) else 0.0, conf_best=c["conf_best"], curves=c,
                                confusion=self.confusion.cpu().numpy().astype(np.int64))
        return out

    def report(self):
        """the report of the statistics `result()` (or `__call__`) last cumulated; see the class docstring.  Needs report=True."""
        if not self.report_on:
            raise RuntimeError("Validator: built with report=False; pass report=True for the losses, curves and confusion matrix")
        if self._report is None:
            self.result()
        return self._report

    def __call__(self):
        from .model import YOLO
        b, N = self.batcher, self.batcher.N
        with torch.cuda.device(self.device), ops.engine_state(self.device):
            blob = self.plan.run(self.ema)
            if self.model is None:
                self.model = YOLO(blob, imgsz=b.s, device=self.device, precision=self.precision)
            else:
                self.model.reload(blob)
            self.reset()
            for b0 in range(0, N, self.batch):
                nb = min(self.batch, N - b0)
                tiles, gl, gb, mk, cnt = (t[:nb] for t in self.bufs[1:])
                b.batch_into(self.table[b0:b0 + nb], tiles, gl, gb, mk, cnt)
                self._label_counts.append(cnt.clone())
                if self.report_on:
                    det, count, head = self.model.predict_tiles(tiles, self.conf, self.iou, self.max_det, return_head=True)
                    self.update(det, count, gl, gb, mk, head=head)
                else:
                    det, count = self.model.predict_tiles(tiles, self.conf, self.iou, self.max_det)
                    self.update(det, count, gl, gb, mk)
                self.tiles = tiles
            out = self.result()
        self.is_best = self.best_fitness is None or out["fitness"] >= self.best_fitness
        if self.is_best:
            self.best_fitness = out["fitness"]
        self.last = out
        return out
