"""The prepare lifecycle the inference models share: a precision (and attention) choice, the prepared state `_prep` keyed by it, and what
invalidates that state.  A class supplies GPU_ONLY (its error message), _prep_device() (the parameter whose device decides) and
_prepare_packed(dev, key, dt), which builds the dict, stores it in self._prep and returns it."""
from .. import hip
from .. import precision as _precision


class Prepared:
    """Mixin in front of torch.nn.Module.  `_prep` is None or the dict of packed weights with its "key"."""
    precision = "fp32"   # the reference's arithmetic; set_precision("fp16") selects the fast mode
    attention = None     # set_precision(..., attention=): None = the attention arithmetic the precision implies
    _prep = None
    HAS_ATTENTION = True    # (the vocoder has no attention: its key is (precision, device))

    def set_precision(self, precision: str, attention=None):
        """'fp16' (f16 MFMA operands, f32 accumulate — fast mode) or 'fp32' (exact-f32 MFMA, parity mode)."""
        # fp32_split: f32 tensors, every Conv1d / Linear but the duration predictor's on split f16 hi/lo MFMA operands (hip.SplitWeight;
        # csrc/conv1d_split.h); fp32_bf16x3 (fp32_bf16x3_6p): the same convs on three exact bf16 terms per operand, seven (six) partial products
        # per product (hip.EmulWeight; csrc/conv1d_emul.h)
        # attention: the self-attention products' arithmetic, a switch of its own.  None (default) = what `precision` has always meant; "fp32_bf16x3" =
        # the seven-product bf16x3 kernel where hip.emul_attention_wins routes it; "fp32" = exact f32.  f32 activations only (not with "fp16").
        hip.check_attention_precision(precision, attention)
        if precision != self.precision or attention != self.attention:
            self.precision, self.attention, self._prep = precision, attention, None
        return self

    def load_state_dict(self, *a, **k):
        self._prep = None
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._prep = None
        return super()._apply(fn, *a, **k)

    def _prepare(self):
        dev = self._prep_device()
        if dev.type != "cuda":
            raise hip._abi.JattsHipError(self.GPU_ONLY)
        key = (self.precision, self.attention, str(dev)) if self.HAS_ATTENTION else (self.precision, str(dev))
        if self._prep is not None and self._prep["key"] == key:
            return self._prep
        hip._abi.load()
        with hip.operands(self.precision), hip.attention_precision(self.attention):
            return self._prepare_packed(dev, key, _precision.TABLE[self.precision].tensors)


class PreparedAcoustic(Prepared):
    """The three acoustic models: created frozen for the inference path, trainable after train(True)."""

    def train(self, mode: bool = True):
        """train(True) also turns the parameters' requires_grad on (they are created frozen for the inference path)."""
        super().train(mode)
        if mode:
            self.requires_grad_(True)
        return self
