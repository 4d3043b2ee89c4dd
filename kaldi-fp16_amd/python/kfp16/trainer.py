"""kfp16.trainer — the chain training step driven by real egs minibatches.

Restates nnet.TrainStep (internal/nnet/train_step.go:142-283) over the build's pieces:
  1. TransferBatch + Forward      -> TrainingBatch.features_to_device (compressed upload,
                                     GPU expansion to fp16) + Network.forward
  2. ComputeChainLossBatch        -> one batched kf_chain_compute; the rows of each eg are
     (chain_loss.go:221-294)         frame_offset + left_context + k * subsampling for
                                     k < frames_per_seq, cut where the eg ends
  3. Backward                     -> Network.backward (seeded at the chain output)
  2a/3b. (TrainConfig.xent_regularize) -> Chain.xent after the objective, then Network.backward with
                                     both seeds: Kaldi's --chain.xent-regularize, which trains the
                                     output-xent branch on the numerator posteriors
  4. optimizer.Update per tensor  -> Network.sgd over the flat buffer (optimize.go:95-142),
                                     or with TrainConfig.kaldi_update Network.update: Kaldi's
                                     per-component max-change, L2 and learning-rate factors
  3a. (TrainConfig.natural_gradient) -> Network.set_natural_gradient: Kaldi's NG-SGD, the weight
                                     gradients preconditioned inside Network.backward
  1a. (TrainConfig.dropout_schedule) -> Network.set_dropout_proportion before the forward: Kaldi's
                                     --trainer.dropout-schedule on the TDNN-F layers' per-sequence
                                     dropout, one mask row per eg
  1b. (TrainConfig.spec_augment)     -> Network.set_spec_augment: Kaldi's SpecAugment on the
                                     spec-augment-layers, one band and one time mask per eg
  1c. (TrainConfig.batchnorm_train)  -> Network.set_batchnorm_train: Kaldi's training-mode BatchNorm
                                     on the sites TrainConfig.batchnorm_train_sites names (the
                                     TDNN-F layers by default; batch statistics, exact backward,
                                     the accumulators commit_batchnorm() later freezes)
  1d. (TrainConfig.row_subsampling)  -> Network.set_row_subsampling(3): the layers above the conv
                                     stack run on the rows the objective reads, which then takes
                                     the output and writes its gradient in compact rows
  2b. (TrainConfig.apply_deriv_weights, example_weights) -> the batch's per-frame deriv weights
                                     and per-eg weights into the objective (Chain.compute's
                                     frame_weight / seq_weight), as Kaldi's trainer applies them
  5. (TrainConfig.orthonormal_every) -> Network.constrain_orthonormal every N-th step: Kaldi's
                                     ConstrainOrthonormal on the TDNN-F bottlenecks
plus, for data parallel, the flat-gradient all-reduce between 3 and 4 (kfp16.dp).

The numerator FSTs come from the batch's per-sequence CSRs (TrainingBatch.PerSeqCSRs),
the denominator from a DenGraph the caller builds (NativeDenominator's transitions).
Everything runs on the GPU; this module only sequences the calls.

A network with Kaldi's ivector input (`input name=ivector`, ReplaceIndex(ivector, t, 0))
gets the batch's per-eg ivectors, expanded on the GPU next to the features, with one
sequence per eg (nnet_forward_ivector). The reference drops them at this point.
"""
from __future__ import annotations

import re
from dataclasses import dataclass

import numpy as np

from . import DeviceBuffer, Network, core, sync
from . import chain as _chain


@dataclass
class TrainConfig:
    """TrainConfig (train_step.go:20-30) fields the step uses."""
    learning_rate: float = 1e-4
    momentum: float = 0.9
    subsampling_factor: int = 3
    left_context: int = 30
    opts: _chain.KfChainOpts | None = None
    # kaldi_update: step 4 is Network.update (per-component max-change / l2-regularize /
    # learning-rate-factor from the xconfig or Network.set_component_opts) with the global
    # max_param_change (0: no limit; Kaldi's recipes use 2.0) and l2_scale (None: the batch's
    # supervised frame count, Kaldi's factor). False: the plain Network.sgd, as before.
    kaldi_update: bool = False
    max_param_change: float = 0.0
    l2_scale: float | None = None
    # orthonormal_every: N > 0 applies the semi-orthogonal constraint (Network.constrain_orthonormal,
    # Kaldi's ConstrainOrthonormal) after the parameter update of every N-th step, with either
    # update; Kaldi handles each component at one update in four on average, which is N = 4.
    # 0: never, as before.
    orthonormal_every: int = 0
    # natural_gradient: Kaldi's NG-SGD (Network.set_natural_gradient with its default options):
    # the backward leaves the preconditioned weight gradients of the linear, output, tdnnf and
    # prefinal components for step 4, with either update. False: plain gradients, as before.
    natural_gradient: bool = False
    # dropout_schedule: Kaldi's --trainer.dropout-schedule, e.g. '0,0@0.20,0.5@0.50,0': the
    # proportion of every layer with a dropout component (xconfig dropout-proportion >= 0) as a
    # piecewise-linear function of the fraction of data processed (dropout_proportion below), set
    # before each forward; one mask row per eg, drawn from dropout_seed (under data parallel each
    # rank folds its rank in, so ranks draw different masks). total_steps: the number of steps the
    # fraction is derived from (steps taken / total_steps) when step() is not given one.
    # '': nothing is called, as before.
    dropout_schedule: str = ""
    dropout_seed: int = 0
    total_steps: int = 0
    # spec_augment: Network.set_spec_augment on the xconfig's spec-augment-layers (Kaldi's
    # frequency and time masks), one sequence per eg, drawn from spec_augment_seed
    # (under data parallel each rank folds its rank in, as for dropout). False: nothing is called.
    spec_augment: bool = False
    spec_augment_seed: int = 0
    # batchnorm_train: Network.set_batchnorm_train at construction: the TDNN-F layers'
    # BatchNorm normalises each minibatch by its own statistics, the backward differentiates
    # through them, and the accumulators start from zero (Kaldi's ZeroComponentStats);
    # EgsTrainer.commit_batchnorm() makes them the frozen statistics. False: frozen, as before.
    batchnorm_train: bool = False
    # batchnorm_train_sites: the layers batchnorm_train governs (Network.set_batchnorm_train_sites,
    # DESIGN §27): "tdnnf", "conv", "prefinal", "batchnorm", comma-separated, or "all" (what Kaldi
    # does). With the default nothing more than before is called.
    batchnorm_train_sites: str = "tdnnf"
    # batchnorm_train_rows: Network.set_batchnorm_train_rows: "all" or "subsampled";
    # the latter is what lets batchnorm_train and row_subsampling be on together. With the default
    # nothing more than before is called.
    batchnorm_train_rows: str = "all"
    # self_repair: Network.set_self_repair after batchnorm_train: Kaldi's ReLU unit
    # statistics on every forward and self-repair on every backward, for the ReLUs batchnorm_train
    # governs, with the xconfig's self-repair-scale (1e-5) and thresholds; the statistics start from
    # zero. Needs batchnorm_train. EgsTrainer.relu_summary() reads the statistics. False: the
    # trainer makes exactly the calls it made before.
    self_repair: bool = False
    # row_subsampling: the row-subsampled step (Network.set_row_subsampling(3) at construction; a
    # topology it does not cover raises there). A step whose subsampling_factor is 3 and whose egs
    # all have their first supervised row at 0 (mod 3) runs the objective on the compact rows; any
    # other batch takes that one step on all rows (counted in EgsTrainer.full_row_steps).
    # False: nothing is called, as before.
    row_subsampling: bool = False
    # xent_regularize: Kaldi's --chain.xent-regularize (the recipes use 0.1). > 0: the
    # value goes into the objective's options, Chain.xent writes the output-xent layer's gradient
    # from the numerator posteriors and the backward takes both seeds; result() then also
    # carries xent_objf and xent_weight. The recipes' learning-rate-factor of the xent layers
    # (0.5 / xent_regularize) is the xconfig key learning-rate-factor, honoured by kaldi_update.
    # 0: the trainer makes exactly the calls it made before.
    xent_regularize: float = 0.0
    # apply_deriv_weights: Kaldi's --apply-deriv-weights (true there): the batch's
    # per-frame deriv weights (<DW> / <DW2>, cut to each eg's supervised frames) scale the rows of
    # the chain derivative and of the xent derivative, inside the objective's kernels.
    # example_weights: each eg's own <Weight> multiplies opts.supervision_weight for its sequence.
    # Both False: the trainer makes exactly the calls it made before.
    apply_deriv_weights: bool = False
    example_weights: bool = False
    # loss_scale: dynamic loss scaling of the fp16 step, kept on the device. > 0 is the
    # initial scale (Network.set_loss_scale; the reference's script trains with 65536): the
    # objective multiplies its derivative by the scale, and step 4 checks the gradient buffer,
    # skips the step and halves the scale on a non-finite value, and unscales otherwise; after
    # loss_scale_growth_interval clean steps the scale doubles (at most 65536). A skipped step
    # still counts in `steps`. Not with natural_gradient. 0: the trainer makes exactly the calls it
    # made before.
    loss_scale: float = 0.0
    loss_scale_growth_interval: int = 2000

    def __post_init__(self):
        if self.self_repair and not self.batchnorm_train:
            raise ValueError("self_repair needs batchnorm_train: its sites are the ReLUs training-mode BatchNorm governs")
        if not (self.loss_scale >= 0.0) or not np.isfinite(self.loss_scale):
            raise ValueError(f"loss_scale {self.loss_scale}: needs a finite value >= 0 (0: off)")
        if self.loss_scale_growth_interval < 1:
            raise ValueError(f"loss_scale_growth_interval {self.loss_scale_growth_interval}: needs >= 1")
        if self.loss_scale > 0 and self.natural_gradient:
            raise ValueError("loss_scale is not supported with natural_gradient: the preconditioner's Fisher "
                             "state is not scale-equivariant across a change of the scale")


def parse_dropout_schedule(schedule: str):
    """[(fraction, proportion)] of Kaldi's 'v0,v1@f1,...,vN' form: the first value is at fraction
    0, the last at 1, the ones between carry their fraction after '@', strictly increasing
    inside (0, 1). Proportions must lie in [0, 0.5] (the continuous mask stays >= 0)."""
    parts = [t.strip() for t in schedule.split(",")]
    if len(parts) < 2 or any(not t for t in parts):
        raise ValueError(f"dropout schedule {schedule!r}: needs at least a first and a last value")
    pts = []
    for i, tok in enumerate(parts):
        ends = i == 0 or i == len(parts) - 1
        if ends == ("@" in tok):
            raise ValueError(f"dropout schedule {schedule!r}: {tok!r} "
                             + ("is an end value and takes no fraction" if ends else "needs value@fraction"))
        try:
            if ends:
                v, f = float(tok), 0.0 if i == 0 else 1.0
            else:
                a, b = tok.split("@")
                v, f = float(a), float(b)
        except ValueError:
            raise ValueError(f"dropout schedule {schedule!r}: cannot read {tok!r}") from None
        if not (0.0 <= v <= 0.5):
            raise ValueError(f"dropout schedule {schedule!r}: proportion {v} outside [0, 0.5]")
        if not ends and not (0.0 < f < 1.0):
            raise ValueError(f"dropout schedule {schedule!r}: fraction {f} outside (0, 1)")
        if pts and f <= pts[-1][0]:
            raise ValueError(f"dropout schedule {schedule!r}: fractions must strictly increase")
        pts.append((f, v))
    return pts


def dropout_proportion(schedule: str, fraction: float) -> float:
    """The proportion Kaldi's dropout schedule gives at `fraction` of the data processed
    (clamped to [0, 1]): piecewise linear between the schedule's points."""
    pts = parse_dropout_schedule(schedule)
    x = min(1.0, max(0.0, float(fraction)))
    for (f0, v0), (f1, v1) in zip(pts, pts[1:]):
        if x <= f1:
            return v0 + (v1 - v0) * (x - f0) / (f1 - f0)
    return pts[-1][1]


def chain_rows(frame_offsets, num_frames, frames_per_seq, subsampling: int, left_context: int):
    """Per-eg (first output row, supervised frames) as ComputeChainLossBatch forms them
    (chain_loss.go:240-255): the eg's view is cut at left_context + fps * subsampling
    input rows, then every subsampling-th row from left_context is taken."""
    row0, frames = [], []
    for off, T, fps in zip(frame_offsets, num_frames, frames_per_seq):
        eff = min(left_context + int(fps) * subsampling, int(T))
        n = max(0, -(-(eff - left_context) // subsampling))  # ceil
        row0.append(int(off) + left_context)
        frames.append(min(int(fps), n))
    return np.asarray(row0, np.int32), np.asarray(frames, np.int32)


class EgsTrainer:
    """One network + objective, stepping on loader.TrainingBatch minibatches."""

    def __init__(self, xconfig: str, den_graph: dict, max_egs: int, max_frames: int,
                 config: TrainConfig | None = None, grad_buffer_ptr: int | None = None, rank: int = 0):
        self.cfg = config or TrainConfig()
        self.net = Network(xconfig, max_frames=max_frames)
        self.P = self.net.layers[[n for n, *_ in self.net.layers].index("output")][3] \
            if any(n == "output" for n, *_ in self.net.layers) else self.net.layers[-1][3]
        self.max_frames = max_frames
        self.feat = DeviceBuffer(max_frames * 40 * 2)
        self.grad_out = DeviceBuffer(max_frames * self.P * 2)
        self.dgraph = _chain.DenGraph(den_graph)
        self.objective = _chain.Chain(self.dgraph, max_seqs=max_egs,
                                      max_frames=max(1, max_frames // self.cfg.subsampling_factor + 1))
        if grad_buffer_ptr is not None:
            self.net.bind_grad_buffer(grad_buffer_ptr)
        self.out_ptr = self.net.activation("output")[0]
        m = re.search(r"^\s*input\s+name=ivector\s+dim=(\d+)", xconfig, re.M)
        self.ivec_dim = int(m.group(1)) if m else 0
        self.ivec = DeviceBuffer(max_egs * self.ivec_dim * 2) if self.ivec_dim else None
        self.max_egs = max_egs
        self.steps = 0  # steps taken
        self.xent_grad = None
        if self.cfg.xent_regularize > 0:
            dims = {n: dout for n, _ty, _din, dout in self.net.layers}
            if dims.get("output-xent") != self.P:
                raise ValueError("xent_regularize needs an output-xent layer as wide as the chain output")
            o = self.cfg.opts or _chain.KfChainOpts.default()
            self.opts = _chain.KfChainOpts(o.l2_regularize, o.out_of_range_regularize, o.leaky_hmm_coefficient,
                                           float(self.cfg.xent_regularize), o.supervision_weight)
            self.xent_ptr = self.net.activation("output-xent")[0]
            self.xent_grad = DeviceBuffer(max_frames * self.P * 2)
        else:
            self.opts = self.cfg.opts
        if self.cfg.natural_gradient:
            self.net.set_natural_gradient(True)
        if self.cfg.dropout_schedule:
            parse_dropout_schedule(self.cfg.dropout_schedule)  # a malformed schedule fails here
            # (each data-parallel rank its own masks: the rank folded into the seed)
            self.net.set_dropout(True, (int(self.cfg.dropout_seed) + 0x9E3779B97F4A7C15 * int(rank)) % 2 ** 64)
        if self.cfg.spec_augment:
            self.net.set_spec_augment(True, (int(self.cfg.spec_augment_seed) + 0x9E3779B97F4A7C15 * int(rank)) % 2 ** 64)
        if self.cfg.batchnorm_train_rows != "all":
            self.net.set_batchnorm_train_rows(self.cfg.batchnorm_train_rows)
        self.full_row_steps = 0  # steps row_subsampling ran on all rows (a batch off the 0 (mod 3) grid, a T too short)
        if self.cfg.row_subsampling:
            self.net.set_row_subsampling(3)
        if self.cfg.batchnorm_train:
            if self.cfg.batchnorm_train_sites != "tdnnf":
                self.net.set_batchnorm_train_sites(self.cfg.batchnorm_train_sites)
            self.net.set_batchnorm_train(True)
            self.net.batchnorm_zero_stats()
        if self.cfg.self_repair:
            self.net.set_self_repair(True)
            self.net.relu_zero_stats()
        if self.cfg.loss_scale > 0:
            self.net.set_loss_scale(True, init_scale=float(self.cfg.loss_scale),
                                    growth_interval=int(self.cfg.loss_scale_growth_interval),
                                    max_scale=max(65536.0, float(self.cfg.loss_scale)))
            self.objective.set_grad_scale(self.net.loss_scale_ptr())

    def relu_summary(self) -> dict:
        """Per self-repair site, what nnet3-info prints of a ReLU: {"count", "deriv_avg_pct": the 5th,
        50th and 95th percentile of deriv-avg, "dead", "saturated": the units at or below the site's
        lower / above its upper threshold, "units"} (synchronises)."""
        out = {}
        for name in self.net.self_repair_sites():
            st, o = self.net.relu_stats(name), self.net.self_repair_opts(name)
            d = st["deriv_avg"]
            live = st["count"] > 0
            out[name] = {"count": st["count"], "units": int(d.size),
                         "deriv_avg_pct": [float(x) for x in np.percentile(d, [5, 50, 95])],
                         "dead": int(np.sum(d <= o["lower"])) if live else 0,
                         "saturated": int(np.sum(d > o["upper"])) if live else 0}
        return out

    def loss_scale_stats(self) -> dict:
        """Network.loss_scale_stats of a trainer with TrainConfig.loss_scale > 0 (synchronises)."""
        return self.net.loss_scale_stats()

    def step(self, batch, allreduce=None, fraction: float | None = None):
        """One TrainStep on `batch` (kfp16.egs.TrainingBatch). allreduce: optional callable
        run between backward and SGD (data parallel). fraction: the fraction of data processed,
        for the dropout schedule (None: steps taken / TrainConfig.total_steps). Asynchronous on
        the library stream; call result() for the objective."""
        T = batch.total_frames
        if T > self.max_frames or batch.feat_dim != 40:
            raise ValueError(f"batch of {T} frames x {batch.feat_dim} does not fit the trainer")
        if self.ivec_dim:
            if batch.ivector_dim != self.ivec_dim or batch.batch_size > self.max_egs:
                raise ValueError(f"batch of {batch.batch_size} egs with {batch.ivector_dim}-dim ivectors does "
                                 f"not fit the trainer's {self.ivec_dim}-dim ivector input")
            batch.features_to_device(self.feat.ptr, 40, self.ivec.ptr)
        else:
            batch.features_to_device(self.feat.ptr, 40)
        rsub = self.cfg.row_subsampling
        if not rsub:
            self._zero_grads(T)
        seq = np.append(np.asarray(batch.frame_offsets, np.int32), np.int32(T))
        if self.cfg.dropout_schedule:
            if fraction is None:
                if self.cfg.total_steps <= 0:
                    raise ValueError("a dropout schedule needs step(fraction=...) or TrainConfig.total_steps")
                fraction = self.steps / self.cfg.total_steps
            self.net.set_dropout_proportion(dropout_proportion(self.cfg.dropout_schedule, fraction))
        if (self.cfg.dropout_schedule or self.cfg.spec_augment) and not self.ivec_dim:
            self.net.set_sequences(seq)
        row0, frames = chain_rows(batch.frame_offsets, batch.num_frames, batch.frames_per_seq,
                                  self.cfg.subsampling_factor, self.cfg.left_context)
        # row subsampling declares that the objective reads rows 0 (mod 3) only: a batch that does
        # not keep to that takes this one step on all rows
        aligned = rsub and self.cfg.subsampling_factor == 3 and bool(np.all(row0 % 3 == 0))
        if rsub and not aligned:
            self.net.set_row_subsampling(0)
        if self.ivec_dim:
            self.net.forward_ivector(self.feat.ptr, T, self.ivec.ptr, seq)
        else:
            self.net.forward(self.feat.ptr, T)
        if rsub and not aligned:
            self.net.set_row_subsampling(3)
        num = _chain.NumBatch(batch.num_fsts())
        # the objective's layout: the forward's frames, or with a compact row set (tc > 0; 0: a T
        # too short for one) its tc rows, where compact row c is frame 3c for every supervised row
        obj_rows, obj_row0, obj_stride = T, row0, self.cfg.subsampling_factor
        if rsub:
            tc, _tc0, _ = self.net.row_set()
            if aligned and tc:
                obj_rows, obj_row0, obj_stride = tc, (row0 // 3).astype(np.int32), 1
            else:
                self.full_row_steps += 1
            self._zero_grads(obj_rows)
        # the weights the egs carry, by (sequence, frame): the same on either row layout
        seq_w = frame_w = None
        if self.cfg.example_weights:
            seq_w = np.asarray(batch.example_weights, np.float32)
        if self.cfg.apply_deriv_weights:
            dw, have = batch.deriv_weights()
            if have:  # an eg cut short keeps its first frames[i] weights
                o = np.concatenate(([0], np.cumsum(np.maximum(batch.frames_per_seq, 0))))
                frame_w = np.concatenate([dw[o[i]:o[i] + frames[i]] for i in range(len(frames))]
                                         or [np.zeros(0, np.float32)]).astype(np.float32)
        if seq_w is None and frame_w is None:
            self.objective.compute(num, self.out_ptr, self.P, obj_rows, obj_row0, frames, obj_stride,
                                   self.grad_out.ptr, self.P, self.opts)
        else:
            self.objective.compute(num, self.out_ptr, self.P, obj_rows, obj_row0, frames, obj_stride,
                                   self.grad_out.ptr, self.P, self.opts, seq_weight=seq_w, frame_weight=frame_w)
        self._num = num  # kept alive until the stream has consumed it
        if self.xent_grad is not None:
            self.objective.xent(num, self.xent_ptr, self.P, self.xent_grad.ptr, self.P, self.opts)
            self.net.backward(self.grad_out.ptr, self.xent_grad.ptr)
        else:
            self.net.backward(self.grad_out.ptr)
        if allreduce is not None:
            allreduce()
        if self.cfg.kaldi_update:
            l2_scale = float(frames.sum()) if self.cfg.l2_scale is None else self.cfg.l2_scale
            self.net.update(self.cfg.learning_rate, self.cfg.momentum, self.cfg.max_param_change, l2_scale)
        else:
            self.net.sgd(self.cfg.learning_rate, self.cfg.momentum)
        self.steps += 1
        if self.cfg.orthonormal_every > 0 and self.steps % self.cfg.orthonormal_every == 0:
            self.net.constrain_orthonormal()

    def _zero_grads(self, rows: int):
        # rows the objective does not write must be zero for this batch
        core.bridge_gpu_memset(self.grad_out.ptr, 0, rows * self.P * 2)
        if self.xent_grad is not None:
            core.bridge_gpu_memset(self.xent_grad.ptr, 0, rows * self.P * 2)

    def result(self):
        """The objective's KfChainResult of the last step; with xent_regularize > 0 it also has
        the attributes xent_objf and xent_weight (Chain.xent_result)."""
        sync()
        r = self.objective.result()
        if self.xent_grad is not None:
            r.xent_objf, r.xent_weight = self.objective.xent_result()
        return r

    def commit_batchnorm(self) -> int:
        """Network.batchnorm_commit: the accumulated statistics of the training-mode BatchNorms
        become the frozen ones (what a model written after this job carries); returns the number
        of layers committed. The mode stays as it is."""
        return self.net.batchnorm_commit()
