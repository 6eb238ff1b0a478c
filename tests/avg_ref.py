"""Float64 restatement of the weight averaging of include/fcosdet.h "Averaging the model's weights" (optim.AveragedModel): the begin rule (apply, weight,
n_averaged for SWA / EMA, the optimizer's skip flag, start_step / every), the update avg + (p - avg) * w with its copy case, and the buffer rule for both
values of use_buffers.  tests/test_avg_cpu.py holds it against torch.optim.swa_utils.AveragedModel in float64; the GPU tests hold the kernels against it."""
import torch

SWA, EMA = 0, 1


def begin(n_averaged, mode, decay=0.0, skip=False, global_step=None, start_step=0, every=1):
    """-> (apply, weight, n_averaged after).  global_step None: no gate (no optimizer)."""
    apply = not skip and (global_step is None or (global_step >= start_step and (global_step - start_step) % every == 0))
    if not apply:
        return False, 0.0, n_averaged
    weight = 1.0 if n_averaged == 0 else (1.0 / float(n_averaged + 1) if mode == SWA else 1.0 - decay)
    return True, weight, n_averaged + 1


def weight_f32(weight):
    """The factor the update launches multiply by: the fp64 weight rounded once to fp32."""
    return float(torch.tensor(weight, dtype=torch.float64).to(torch.float32))


def update(avg, p, weight):
    """One tensor in float64: a copy when the weight is 1, else avg + (p - avg) * w."""
    if weight == 1.0:
        return p.clone()
    return avg + (p - avg) * weight


def gate_schedule(steps, start_step, every, skipped=()):
    """The steps of `steps` on which an update applies."""
    return [g for g in steps if begin(0, SWA, skip=g in skipped, global_step=g, start_step=start_step, every=every)[0]]


class RefAveraged:
    """The averaged copy of a list of parameters and a list of buffers, in float64 (integer buffers keep their dtype).  update(...) takes the model's current
    tensors; `rounded` = the weight goes through fp32 as on the device."""

    def __init__(self, params, buffers=(), mode=SWA, decay=0.0, use_buffers=False, start_step=0, every=1, rounded=False):
        self.p = [self._f64(t) for t in params]
        self.b = [self._f64(t) for t in buffers]
        self.mode, self.decay, self.use_buffers, self.start_step, self.every, self.rounded = mode, decay, use_buffers, start_step, every, rounded
        self.n_averaged = 0

    @staticmethod
    def _f64(t):
        return t.detach().to(torch.float64).clone() if t.is_floating_point() else t.detach().clone()

    def update(self, params, buffers=(), skip=False, global_step=None):
        apply, w, self.n_averaged = begin(self.n_averaged, self.mode, self.decay, skip, global_step, self.start_step, self.every)
        if not apply:
            return False
        if self.rounded:
            w = weight_f32(w)
        self.p = [update(a, self._f64(p), w) for a, p in zip(self.p, params)]
        # buffers: copied on every applied call without use_buffers; with it the floating ones are averaged and the integer ones copied
        self.b = [update(a, self._f64(b), w) if (self.use_buffers and b.is_floating_point()) else self._f64(b) for a, b in zip(self.b, buffers)]
        return True
