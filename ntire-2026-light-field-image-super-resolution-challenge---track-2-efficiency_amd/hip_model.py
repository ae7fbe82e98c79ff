"""What the model plugins (model/SR/*.py) share: the module tree of a plugin is a parameter container only, and
``forward`` hands the tensors to the gfx950 HIP library through the C ABI (lfsr_amd.capi); none of the
``nn.Module.forward`` paths of the containers is ever executed and there is no CPU fallback.

Weights: the runtime holds packed copies of the parameters.  A no-grad forward repacks when a parameter's ``(data_ptr, _version)``
moved (``load_state_dict``, ``.to()``, an optimizer step).  Every training forward repacks, because an optimizer may update the values
without bumping ``p._version`` (``AdamW(fused=True)`` does), and it clears the inference key, so the next no-grad forward repacks too.
Writes that bypass the version counter (``p.data.copy_``, collectives on ``p.data``) must be followed by ``invalidate_packed()``.
"""
import torch
import torch.nn as nn

from lfsr_amd import capi


class _Holder(nn.Module):
    """Parameter container whose forward must never run."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container: the HIP path computes this layer")


class _HipModelFunction(torch.autograd.Function):
    """Whole-model autograd node: forward and backward both run in the HIP library; the gradients of all parameters come back as
    views of ONE flat fp32 bucket (``model.grad_bucket``) ready for a single all-reduce."""

    @staticmethod
    def forward(ctx, model, x, *params):
        rt = model._train_runtime(x.device)
        ctx.model, ctx.rt = model, rt
        ctx.save_for_backward(x)
        out = rt.forward_train(x)
        ctx.generation = rt.train_generation      # the saved activations live in the runtime's ONE training workspace
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        model, rt = ctx.model, ctx.rt
        if ctx.generation != rt.train_generation:
            raise capi.LfsrError(f"{model.hip_name} backward: a later forward (with grad enabled) has overwritten the training workspace this "
                                 "graph's activations lived in; run backward before the next training forward")
        # A FRESH bucket per backward: autograd's AccumulateGrad keeps (steals) the tensors returned here as p.grad, so handing it
        # views of a buffer that the next backward overwrites would make `p.grad += new` run on aliased memory (zero_grad(set_to_none=
        # False) or gradient accumulation would silently double the gradients).  model.grad_bucket is the latest one.
        bucket = torch.empty(rt.num_params(), dtype=torch.float32, device=x.device)
        rt.backward(x, dout, bucket)
        model.grad_bucket = bucket
        grads = []
        for name, p in model.named_parameters():
            off, n = model._spans[name]
            grads.append(bucket[off:off + n].view_as(p) if p.requires_grad else None)
        return (None, None, *grads)


class HipModel(nn.Module):
    """Base of a plugin's ``get_model``: owns the runtime (``_rt``), its repack key and the dispatch of ``forward``.
    A subclass builds its module tree after ``super().__init__()`` and implements ``_new_runtime``."""

    hip_name = None           # the model's name in error texts
    trainable = True          # False: the C ABI has no training symbols for the model, a forward with grad enabled is refused

    def __init__(self):
        super().__init__()
        self._rt = None
        self._rt_version = None
        self._spans = None
        self.grad_bucket = None      # flat fp32 gradient bucket filled by the HIP backward (state_dict order)

    def _new_runtime(self):
        raise NotImplementedError

    def _repack(self, device):
        self._rt.load_state(self.state_dict().items(), device)

    def _runtime(self, device):
        if self._rt is None:
            self._rt = self._new_runtime()
        ver = (device, tuple((p.data_ptr(), p._version) for p in self.parameters()))
        if ver != self._rt_version:
            self._repack(device)
            self._rt_version = ver
        return self._rt

    def _train_runtime(self, device):
        """every training forward repacks and clears the inference key (see the module docstring)"""
        if self._rt is None:
            self._rt = self._new_runtime()
        if self._spans is None:
            self._spans = {k: self._rt.param_span(k) for k, _ in self.named_parameters()}
        self._repack(device)
        self._rt_version = None
        return self._rt

    def invalidate_packed(self):
        """Force a repack at the next forward (for weight writes that bypass p._version: ``p.data.copy_``, collectives)."""
        self._rt_version = None

    def forward(self, x, info=None):
        if not x.is_cuda:
            raise capi.LfsrError(f"{self.hip_name}: input must live on the MI355X (no CPU fallback in the HIP path)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if not self.trainable:
                raise capi.LfsrError(f"{self.hip_name} is inference-only on the HIP path (no backward behind the C ABI): run the forward under "
                                     "torch.no_grad(), or freeze the parameters")
            return _HipModelFunction.apply(self, x.float(), *self.parameters())      # train.py:257
        return self._runtime(x.device).forward(x.float())
