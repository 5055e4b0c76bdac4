"""Host-side mirror of /root/reference/models/search/ntu_searchable.py for the HIP engine.

Same names, argument meaning and error behaviour as the reference for the hot path:

* ``train_sampled_models``               ntu_searchable.py:23-102   (population loop -> lockstep engine; mfas_amd/driver.py)
* ``get_possible_layer_configurations``  ntu_searchable.py:105-119
* ``get_central_states`` / ``set_central_states``   ntu_searchable.py:123-174   (weight sharing; mfas_amd/driver.py)
* ``Searchable_Skeleton_Image_Net``      ntu_searchable.py:178-301  (nn.Module surface)

This file holds the nn.Module surface; the driver's names (mfas_amd/driver.py) are re-exported below as the same objects (PROFILE,
RUNG_CHANGES, _DEVICE_STREAMS_OK are mutated in place).  A module attribute the driver READS (_TEST_FAIL_RANK) is set on mfas_amd.driver.

Departures: backbones are feature tables (``FeatureTap`` stands in for
``Visual``/``Skeleton``; north_star: precomputed features); candidates of one call train in
lockstep and share the epoch's batch order; dropout uses the engine's counter-based stream.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .driver import (PROFILE, ROUNDS_MIN_CANDIDATES, RUNG_CHANGES, _DEVICE_STREAMS_OK, _bump_bn_counters,  # noqa: F401
                     _check_halving, _init_population_device_streams, _init_population_from_torch, _plan_rounds, _require_loader,
                     get_central_states, initial_flat_params, make_order, make_order_per_candidate, set_central_states,
                     torch_init_bounds, train_sampled_models)
from .engine import FeatureTable, Hyper, Population, flat_layout


# ------------------------------------------------------------------------------------------------ small modules
class GlobalPooling2D(nn.Module):
    """models/auxiliary/aux_models.py:54-64: mean over all trailing dims (identity on pooled (B,C) taps)."""

    def forward(self, x):
        x = x.view(x.size(0), x.size(1), -1)
        return torch.mean(x, 2).view(x.size(0), -1)


class AlphaScalarMultiplication(nn.Module):
    """aux_models.py:94-111: x*sigmoid(alpha), y*(1-sigmoid(alpha)); one scalar per cell.  The arithmetic
    runs inside the engine; this module only owns the parameter."""

    def __init__(self, size_alpha_x, size_alpha_y):
        super().__init__()
        self.size_alpha_x = size_alpha_x
        self.size_alpha_y = size_alpha_y
        self.alpha_x = nn.Parameter(torch.zeros(1, dtype=torch.float32))


class FeatureTap(nn.Module):
    """Stand-in for the frozen backbones ``Visual`` / ``Skeleton`` (models/central/ntu.py:17,53): the
    taps are precomputed, so this module has no parameters and simply hands the batch's taps on."""

    def __init__(self, prefix):
        super().__init__()
        self.prefix = prefix

    def forward(self, x):
        return x


class _TrainModeForward(torch.autograd.Function):
    """Train-mode forward of one batch on the engine WITH an autograd edge to the central parameters: forward =
    mfas_population_forward_train on a scratch population holding the module's parameters; backward = mfas_population_backward on
    a scratch population of the same state (same dropout stream, same batch statistics) with the incoming dL/dlogits — the
    engine's own fused backward, not a torch graph.  ntu_searchable.py:206-247 under model.train(True), for callers that write
    their own loop.  With args.engine_tap_grads the tap tensors that require grad are inputs too, and backward =
    mfas_population_backward_taps for exactly those taps.  Nothing of the GPU is kept between the two calls (the backward pass runs the batch again anyway): a forward
    under no_grad, or one whose loss is never backpropagated, holds no device memory."""

    @staticmethod
    def _scratch(module, table, n, seed, flat0):
        hp = module.hyper(False)
        hp.B = max(n, 2)
        pop = Population(hp, [module.conf], table.label.device, drop_seeds=[seed & 0xFFFFFFFF])
        pop.set_params(0, flat0)
        return pop

    @staticmethod
    def forward(ctx, module, table, n, seed, *rest):
        # rest: the module's parameters, then — engine_tap_grads — a _TapInputs marker and the tap tensors it names
        mark = next((i for i, r in enumerate(rest) if isinstance(r, _TapInputs)), len(rest))
        flat0 = module.flat_params()
        pop = _TrainModeForward._scratch(module, table, n, seed, flat0)
        try:
            out = pop.forward_train(0, table, 0, n, step=0)
            if module.args.batchnorm:
                module.load_flat(pop.get_params(0))      # the moved running statistics (nothing else changed)
                _bump_bn_counters(module, 1)
        finally:
            pop.close()
        ctx.table, ctx.n, ctx.seed, ctx.flat0, ctx.module = table, n, seed, flat0, module
        ctx.tap_names = rest[mark].names if mark < len(rest) else ()
        ctx.tap_like = [(t.dtype, tuple(t.shape)) for t in rest[mark + 1:]]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        module = ctx.module
        want = [name for name, need in zip(ctx.tap_names, ctx.needs_input_grad[-len(ctx.tap_names):]) if need] if ctx.tap_names else []
        pop = _TrainModeForward._scratch(module, ctx.table, ctx.n, ctx.seed, ctx.flat0)     # the state the forward saw
        try:
            if want:      # exactly the taps that ask for a gradient (mfas_population_backward_taps)
                gflat, gtaps = pop.backward_taps(0, ctx.table, grad_out, 0, ctx.n, step=0, taps=want)
                gflat = gflat.cpu()
            else:
                gflat, gtaps = pop.backward(0, ctx.table, grad_out, 0, ctx.n, step=0).cpu(), {}
        finally:
            pop.close()
        where = {key: (shape, off) for key, shape, off in flat_layout(module.conf, module.hyper(False))[0]}
        grads = []
        for key, prm in module.named_parameters():
            # (alphas.parameters() sit in the optimiser but never see a gradient without --alphas, ntu_searchable.py:251)
            if key not in where or (key.startswith("alphas") and not module.args.alphas):
                grads.append(None)
                continue
            shape, off = where[key]
            grads.append(gflat[off:off + int(np.prod(shape))].reshape(shape).to(prm.device))
        if not ctx.tap_names:
            return (None, None, None, None, *grads)
        # each tap's gradient in the tap's own dtype and shape
        tap_grads = [gtaps[name].to(dtype).reshape(shape) if name in gtaps else None for name, (dtype, shape) in zip(ctx.tap_names, ctx.tap_like)]
        return (None, None, None, None, *grads, None, *tap_grads)


class _TapInputs:
    """Marks where the tap tensors begin in _TrainModeForward's arguments, and names them."""

    def __init__(self, names):
        self.names = tuple(names)


# ------------------------------------------------------------------------------------------------ the fusion net
class Searchable_Skeleton_Image_Net(nn.Module):
    """Module surface of ntu_searchable.py:178-301: attributes ``conf, args, rgbnet, skenet, alphas, gp_v,
    gp_s, fusion_layers, central_classifier``; ``forward``; ``central_params``.

    conf: one row per fusion cell: [ske tap, rgb tap, non-linearity (0 ReLU / 1 Sigmoid / 2 LeakyReLU)].
    """
    # construction draws torch's generator exactly like initial_flat_params restates it (per cell Linear weight, bias; classifier;
    # then the alphas): train_sampled_models may then initialise candidates of this class without building modules.  A subclass that
    # constructs differently (other layers, another order) sets this to False.
    _construction_is_standard = True

    def __init__(self, args, conf):
        super().__init__()
        self.conf = np.asarray(conf)
        self.args = args
        self.rgbnet = FeatureTap("v")
        self.skenet = FeatureTap("s")
        self.alphas = self._create_alphas()
        self.gp_v, self.gp_s = self._create_global_poolings()
        self.fusion_layers = self._create_fc_layers()
        self.central_classifier = nn.Linear(self.args.inner_representation_size, args.num_outputs)
        for m in self.modules():
            if isinstance(m, AlphaScalarMultiplication):
                nn.init.normal_(m.alpha_x, 0.0, 0.1)
        self._pop = None

    # -- construction (ntu_searchable.py:258-301)
    def _sizes(self):
        hp = Hyper.from_args(self.args)
        return hp.s_sizes, hp.v_sizes

    def _create_alphas(self):
        sizes_ske, sizes_ims = self._sizes()
        return nn.ModuleList([AlphaScalarMultiplication(sizes_ske[int(c[0])], sizes_ims[int(c[1])])
                              for c in self.conf])

    def _create_global_poolings(self):
        n = len(self.conf)
        return (nn.ModuleList([GlobalPooling2D() for _ in range(n)]),
                nn.ModuleList([GlobalPooling2D() for _ in range(n)]))

    def _create_fc_layers(self):
        layers = []
        for i, conf in enumerate(self.conf):
            in_size = self.alphas[i].size_alpha_x + self.alphas[i].size_alpha_y
            if i > 0:
                in_size += self.args.inner_representation_size
            out_size = self.args.inner_representation_size
            if conf[2] == 0:
                nl = nn.ReLU()
            elif conf[2] == 1:
                nl = nn.Sigmoid()
            elif conf[2] == 2:
                nl = nn.LeakyReLU()
            else:
                raise ValueError(f"unknown non-linearity {conf[2]}")
            drop, bn = self.args.drpt > 1e-10, bool(self.args.batchnorm)
            if drop and bn:
                op = nn.Sequential(nn.Linear(in_size, out_size), nl, nn.BatchNorm1d(out_size),
                                   nn.Dropout(self.args.drpt))
            elif drop:
                op = nn.Sequential(nn.Linear(in_size, out_size), nl, nn.Dropout(self.args.drpt))
            elif bn:
                op = nn.Sequential(nn.Linear(in_size, out_size), nl, nn.BatchNorm1d(out_size))
            else:   # the reference leaves `op` unassigned here (UnboundLocalError, :274-284)
                raise ValueError("drpt < 1e-10 without --batchnorm is not a legal cell "
                                 "(reference: UnboundLocalError at ntu_searchable.py:284)")
            layers.append(op)
        return nn.ModuleList(layers)

    def central_params(self):
        return [{"params": self.alphas.parameters()},
                {"params": self.fusion_layers.parameters()},
                {"params": self.central_classifier.parameters()}]

    # -- engine plumbing
    def hyper(self, multitask=None) -> Hyper:
        hp = Hyper.from_args(self.args)
        if multitask is not None:
            hp.multitask = bool(multitask)
        return hp

    def flat_params(self) -> torch.Tensor:
        layout, n = flat_layout(self.conf, self.hyper())
        sd = self.state_dict()
        flat = torch.zeros(n, dtype=torch.float32)
        for key, shape, off in layout:
            flat[off:off + int(np.prod(shape))] = sd[key].detach().reshape(-1).to("cpu", torch.float32)
        return flat

    def load_flat(self, flat: torch.Tensor):
        layout, _ = flat_layout(self.conf, self.hyper())
        sd = self.state_dict()
        flat = flat.detach().cpu()
        with torch.no_grad():
            for key, shape, off in layout:
                sd[key].copy_(flat[off:off + int(np.prod(shape))].reshape(shape))

    def _engine(self, device, multitask):
        hp = self.hyper(multitask)
        key = (str(device), hp.multitask)
        if self._pop is None or self._pop[0] != key:
            self._pop = (key, Population(hp, [self.conf], device))
        return self._pop[1]

    def forward(self, tensor_tuple):
        """tensor_tuple = (rgb, ske): dict-likes holding the pooled taps v0..v3 [+ 'vlogit'] and s0..s3
        [+ 'slogit'] on a HIP device.  Eval mode: running-statistics BatchNorm, no Dropout (mfas_population_forward).  Train mode:
        one batch of <= 128 samples with batch statistics and Dropout, differentiable with respect to the central parameters
        (_TrainModeForward).  The taps are outputs of frozen backbones here (feature tables): no gradient flows into them, and
        taps that require grad are refused instead of being silently cut off — unless args.engine_tap_grads is set (opt-in): then
        the engine's backward returns their gradients too, each in the tap's own dtype and shape.  The fast path for training stays
        train_sampled_models / train_ntu_track_acc."""
        image, skeleton = tensor_tuple[0], tensor_tuple[1]
        visual = self.rgbnet(image)
        skel = self.skenet(skeleton)
        taps = {k: v for k, v in visual.items() if k[0] == "v" and k[1:].isdigit()}
        taps.update({k: v for k, v in skel.items() if k[0] == "s" and k[1:].isdigit()})
        if not taps:
            raise ValueError("forward needs the pooled taps 'v0'.. / 's0'.. of the batch (there are no backbones in this engine)")
        some = next(iter(taps.values()))
        n = some.shape[0]
        tap_grads = self.training and torch.is_grad_enabled() and any(t.requires_grad for t in taps.values())
        if tap_grads and not getattr(self.args, "engine_tap_grads", False):
            raise NotImplementedError("the taps require grad, but this engine's backbones are frozen feature tables: it produces gradients "
                                      "for central_params() only (train_only_central_params, ntu_searchable.py:27); detach() the taps")
        # (args.engine_tap_grads, opt-in: the engine's backward also returns the gradients of the taps that require grad —
        #  mfas_population_backward_taps — so the module can sit behind a backbone, adapter or projection that learns)
        live = {k: v for k, v in taps.items() if v.requires_grad} if tap_grads else {}
        # (eval mode needs no gradient of the taps: the reference's eval forward accepts them, so they are detached silently)
        taps = {k: v.detach() for k, v in taps.items()}
        table = FeatureTable(taps, torch.zeros(n, dtype=torch.int32, device=some.device))
        if self.training:
            # train mode (ntu_searchable.py:206-247 under model.train(True)): batch-statistics BatchNorm — running statistics and
            # num_batches_tracked move — and Dropout (the engine's counter-based stream, seeded from torch's RNG).  The logits carry
            # an autograd edge to the central parameters (_TrainModeForward: loss.backward() runs the engine's fused backward);
            # the fast path for training stays train_ntu_track_acc / train_sampled_models.
            if not 1 <= n <= 128:
                raise NotImplementedError("train-mode forward handles one batch of 1..128 samples (the engine's batch range)")
            if n == 1 and self.args.batchnorm:
                raise ValueError("Expected more than 1 value per channel when training")     # torch BatchNorm1d's message
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
            tap_args = (_TapInputs(live), *live.values()) if live else ()
            out = _TrainModeForward.apply(self, table, n, seed, *[p for _, p in self.named_parameters()], *tap_args)
            if not self.args.multitask:
                return out
            return out, visual["vlogit"], skel["slogit"]
        pop = self._engine(some.device, False)
        pop.set_params(0, self.flat_params())
        out = pop.forward(0, table)
        if not self.args.multitask:
            return out
        return out, visual["vlogit"], skel["slogit"]


# ------------------------------------------------------------------------------------------------ search helpers
def get_possible_layer_configurations(progression_index):
    """ntu_searchable.py:105-119: the (4,4,2) grid, non-linearity fastest."""
    max_labels = (4, 4, 2)
    return [[ti, vi, ni] for ti in range(max_labels[0]) for vi in range(max_labels[1])
            for ni in range(max_labels[2])]
