"""Restatement of the dynamic loss scale's rule (kf_ops.h kf_loss_scale_*) in
numpy float32, for the tests: the reference's LossScaler (kaldi_bridge.h kaldi_loss_scaler_update)
with its constants as options. Nothing here touches a device."""
import numpy as np

F32 = np.float32

DEFAULTS = dict(init_scale=65536.0, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=65536.0)


class LossScaleRef:
    """state: scale, since, steps, skipped, last_overflow; inv_used and skip as the update sees them"""

    def __init__(self, **opts):
        o = dict(DEFAULTS, **opts)
        unknown = set(o) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unknown options {sorted(unknown)}")
        self.growth, self.backoff = F32(o["growth"]), F32(o["backoff"])
        self.min_scale, self.max_scale = F32(o["min_scale"]), F32(o["max_scale"])
        self.growth_interval = int(o["growth_interval"])
        self.scale = min(max(F32(o["init_scale"]), self.min_scale), self.max_scale)
        self.inv_used = F32(1) / self.scale
        self.since = self.steps = self.skipped = 0
        self.skip = self.last_overflow = False

    def set_scale(self, scale):
        self.scale = min(max(F32(scale), self.min_scale), self.max_scale)
        self.since = 0

    def update(self, overflow: bool):
        """one step: the check's answer in, the state advanced; returns whether the step is skipped"""
        self.inv_used = F32(1) / self.scale  # latched before the state moves
        self.skip = self.last_overflow = bool(overflow)
        self.steps += 1
        if overflow:
            self.skipped += 1
            self.scale = max(self.min_scale, F32(self.scale * self.backoff))
            self.since = 0
        else:
            self.since += 1
            if self.since >= self.growth_interval:
                self.scale = min(self.max_scale, F32(self.scale * self.growth))
                self.since = 0
        return self.skip

    def stats(self) -> dict:
        return dict(scale=float(self.scale), since=self.since, steps=self.steps, skipped=self.skipped,
                    last_overflow=self.last_overflow)


def overflow_of(g, segments) -> bool:
    """the check's decision: any non-finite element inside the segments [(begin, end)]"""
    g = np.asarray(g)
    return not all(np.isfinite(g[b:e]).all() for b, e in segments)
