"""`torch.nn.Module` surface of the engine classes.

The reference declares `class UniDepthV2(nn.Module, PyTorchModelHubMixin, library_name="UniDepth", ...)`
(unidepth/models/unidepthv2/unidepthv2.py:111-117; V1: unidepthv1/unidepthv1.py:97-103).  Code written against it may type-check the model
(`isinstance(model, nn.Module)`), call it (`model(rgb)`), walk `.parameters()` / `.modules()`, cast it (`.half()`), or `push_to_hub`.
The engine holds its weights as repacked device buffers behind the C-ABI, not as `nn.Parameter`s, so this base gives those calls a defined
meaning instead of an AttributeError:

* `isinstance(model, torch.nn.Module)` holds; `parameters()` / `buffers()` are empty (nothing is trainable here: inference engine);
* `model(...)` = `forward(...)` = `infer(...)`; with a dict first argument (`model(inputs, image_metas)`) it is `forward_test(...)`;
* `.half() / .float() / .double() / .bfloat16() / .to(dtype)` are no-ops with a warning: operand precision is part of the kernels
  (fp16 MFMA operands, fp32 statistics and residual streams), not a property of stored tensors;
* `.train()` raises for `mode=True` (there is no backward), `.eval()` / `.train(False)` return self, `requires_grad_()` is a no-op;
* `state_dict()` returns the fp32 dict with the REFERENCE's key names (what was loaded), `load_state_dict` keeps the engine's chaining
  return value (`model.load_state_dict(sd).to("cuda")`);
* with huggingface_hub importable the classes also derive from `PyTorchModelHubMixin`, so `push_to_hub` exists and goes through the
  engine's own `save_pretrained` (config.json + model.safetensors, the layout `from_pretrained` of both implementations reads).
"""
from __future__ import annotations

import collections
import json
import os
import warnings

import torch

try:                                                    # the reference's second base class; optional here
    from huggingface_hub import PyTorchModelHubMixin as _HubMixin
except Exception:                                       # pragma: no cover - huggingface_hub missing
    class _HubMixin:                                    # type: ignore[no-redef]
        def __init_subclass__(cls, **kwargs):
            super().__init_subclass__()


def _is_batch_dict(args, kwargs) -> bool:
    """The reference's validation call `model(batch["data"], batch["img_metas"])`: a dict where infer() takes the image tensor."""
    return isinstance(args[0] if args else kwargs.get("inputs"), dict)


class EngineModule(torch.nn.Module, _HubMixin):
    """Common nn.Module plumbing of UniDepthV1 / UniDepthV2 (see the module docstring)."""

    def __init__(self):
        super().__init__()
        self.training = False
        self._device = torch.device("cpu")
        self._sd = None                                   # the reference's state_dict, fp32 on the host
        self._w = None                                    # packed device weights (_ensure_packed)
        self._plans: "collections.OrderedDict" = collections.OrderedDict()   # LRU of recorded plans, most recent last; bound: self.max_plans

    # ---- device / dtype ------------------------------------------------------------------------------------------------
    @property
    def device(self):
        return self._device

    def _move(self, device: torch.device) -> None:       # packed weights and plans belong to a device (and to the weights: load_state_dict)
        self._w = None
        self._plans.clear()

    def to(self, *args, **kwargs):
        device = kwargs.get("device")
        dtype = kwargs.get("dtype")
        for a in args:
            if isinstance(a, torch.dtype):
                dtype = a
            elif isinstance(a, bool):
                continue                                    # positional non_blocking (nn.Module.to(device, dtype, non_blocking)): nothing to do
            elif isinstance(a, (str, torch.device, int)):
                device = a
            elif isinstance(a, torch.Tensor):
                device, dtype = a.device, a.dtype
        if dtype is not None:
            self._dtype_noop(f"to({dtype})")
        if device is not None:
            device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
            if device.type == "cuda" and device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            if device != self._device:
                self._device = device
                self._move(device)
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def cpu(self):
        return self.to("cpu")                             # allowed (weights stay on the host anyway); infer() then raises: no CPU path

    def _dtype_noop(self, what: str):
        warnings.warn(f"{type(self).__name__}.{what}: no-op -- the MI355X engine fixes operand precision inside its kernels "
                      "(fp16 MFMA operands, fp32 accumulation / statistics); stored weights stay fp32 and are repacked on .to('cuda')")
        return self

    def half(self):
        return self._dtype_noop("half()")

    def float(self):
        return self._dtype_noop("float()")

    def double(self):
        return self._dtype_noop("double()")

    def bfloat16(self):
        return self._dtype_noop("bfloat16()")

    # ---- mode ------------------------------------------------------------------------------------------------------------
    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError(f"{type(self).__name__} is an inference engine (forward kernels only): train(True) is not available")
        self.training = False
        return self

    def eval(self):
        return self.train(False)

    def requires_grad_(self, requires_grad: bool = True):
        return self

    # ---- call path -------------------------------------------------------------------------------------------------------
    def forward(self, *args, **kwargs):
        """`model(rgb, camera)` runs infer(); `model(inputs, image_metas)` with a dict first argument is the reference's eval-mode
        forward(inputs, image_metas) = forward_test (its training-time forward has no counterpart here)."""
        if _is_batch_dict(args, kwargs):
            return self.forward_test(*args, **kwargs)
        return self.infer(*args, **kwargs)

    # ---- weights (HF mixin layout: config.json + model.safetensors / pytorch_model.bin) -----------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, **kwargs):
        path = str(pretrained_model_name_or_path)
        if not os.path.isdir(path):
            from huggingface_hub import snapshot_download     # e.g. "lpiccinelli/unidepth-v2-vitl14" (needs network / cache)
            path = snapshot_download(path, allow_patterns=["config.json", "model.safetensors", "pytorch_model.bin"])
        with open(os.path.join(path, "config.json")) as f:
            config = json.load(f)
        model = cls(config)
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        return model.load_state_dict(sd)

    def load_state_dict(self, state_dict: dict, strict: bool = False):
        if "model" in state_dict and not torch.is_tensor(state_dict["model"]):
            state_dict = state_dict["model"]                                            # unidepthv2.py:386-388, unidepthv1.py:381-385
        self._sd = {k.replace("module.", ""): v.detach().float().cpu() for k, v in state_dict.items()}
        self._move(self._device)                          # everything derived from the old weights goes
        return self

    def _pack(self) -> dict:                              # subclasses: the packed device weights of self._sd
        raise NotImplementedError

    def _ensure_packed(self):
        if self._device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} (MI355X engine) runs on a ROCm GPU only: call .to('cuda') first; there is no CPU path")
        if self._sd is None:
            raise RuntimeError("no weights loaded (use from_pretrained or load_state_dict)")
        if self._w is None:
            with torch.cuda.device(self._device):
                self._w = self._pack()

    # ---- plan cache ------------------------------------------------------------------------------------------------------
    def _cached_plan(self, key, build):
        """The plan cached under `key`, or `build()` (under the model's device).  A plan owns the full activation set of its signature
        (~2.6 GB for ViT-L at bs=8): the cache is an LRU of `max_plans` entries, so a stream of many image shapes (KITTI / nuScenes
        style) cannot grow device memory without bound."""
        plan = self._plans.get(key)
        if plan is not None:
            self._plans.move_to_end(key)
            return plan
        self._evict_plans(max(1, self.max_plans) - 1)
        with torch.cuda.device(self._device):
            plan = build()
        self._plans[key] = plan
        return plan

    def _evict_plans(self, keep: int):
        """Evict least-recently-used plans down to `keep`.  An evicted plan's buffers go back to the caching allocator of whatever stream
        allocated them, while its launch program may still be queued on ANOTHER stream (pipeline slots): drain the device first -- rare,
        and a plan rebuild costs far more than this sync."""
        if len(self._plans) > keep:
            if self._device.type == "cuda":
                torch.cuda.synchronize(self._device)
            while len(self._plans) > keep:
                self._plans.popitem(last=False)

    def clear_plans(self):
        """Drop every cached launch plan (device activation buffers of all signatures seen so far; rebuilt on the next call)."""
        self._evict_plans(0)

    def state_dict(self, *args, **kwargs):
        """fp32 tensors under the reference's key names (exactly what load_state_dict received, `module.` prefixes stripped)."""
        sd = getattr(self, "_sd", None)
        return dict(sd) if sd is not None else {}

    def save_pretrained(self, save_directory, *, config=None, repo_id=None, push_to_hub: bool = False, **push_to_hub_kwargs):
        """HF layout (config.json + model.safetensors); the keyword arguments are the ones PyTorchModelHubMixin.push_to_hub passes."""
        import json
        import os
        from safetensors.torch import save_file
        save_directory = str(save_directory)
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(self.config, f)
        save_file({k: v.contiguous() for k, v in self._sd.items()}, os.path.join(save_directory, "model.safetensors"))
        if push_to_hub and hasattr(super(), "push_to_hub"):
            kw = dict(push_to_hub_kwargs)
            return super().push_to_hub(repo_id=repo_id or os.path.basename(save_directory.rstrip("/")), **kw)
        return None
