"""What the Python faces of the fetch units (dict_tts_amd/csrc: one ``dtts_text2mel_fetch`` item each) share: the context they run in."""
import torch

from . import abi


class DeviceUnit:
    """A unit keeps ``ctx`` (an existing ``abi.Context``, or None for one of its own) and reaches the device through ``_context()`` only:
    the context is created on the first call, so that argument errors surface without a GPU.  A unit with weights names their tensor
    prefix and part; they are loaded and finalised once, on the first call too."""

    PREFIX = None   # "<PREFIX>.<name>" are the unit's tensors, and
    PART = None     # abi.PART_* is what finalises them (None: the unit loads nothing here)
    ctx = None
    device = None
    _loaded = False

    def _state(self):
        """name -> array of the tensors to load; called before anything touches the device, so a unit may refuse here"""
        return self.weights

    def _device(self):
        """the refusal without a GPU, the device, the context; no weights yet"""
        if self.device is None:
            if not torch.cuda.is_available():
                raise abi.DttsError(f"{type(self).__module__}.{type(self).__name__} needs a ROCm GPU: the HIP path has no CPU fallback")
            self.device = torch.device("cuda", torch.cuda.current_device())
            if self.ctx is None:
                self.ctx = abi.Context()
        return self.ctx

    def _context(self):
        state = self._state() if self.PART is not None and not self._loaded else None
        self._device()
        if state is not None:
            self.ctx.load_state_dict(self.PREFIX, state)
            self.ctx.finalize(self.PART)
            self._loaded = True
        return self.ctx
