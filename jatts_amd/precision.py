"""The inference precisions: one record per name.  Pure Python (dtype codes from _abi; no GPU, no torch).

``tensors`` is the dtype code of the activations in HBM, ``operand`` the operand code of a `dtype=F32` conv call site (hip.f32_operand):
F32S = split f16 hi/lo MFMA operands (hip.SplitWeight), F32E / F32E6 = three exact bf16 terms per operand, seven / six partial products
(hip.EmulWeight).  Everything else that depends on a precision name derives from these two fields."""
from typing import NamedTuple

from ._abi import F16, F32, F32E, F32E6, F32S

EMUL = (F32E, F32E6)


class Precision(NamedTuple):
    tensors: int
    operand: int

    @property
    def split(self):
        return self.operand == F32S

    @property
    def emul(self):
        return self.operand in EMUL


TABLE = {
    "fp16": Precision(F16, F16),
    "fp32": Precision(F32, F32),
    "fp32_split": Precision(F32, F32S),
    "fp32_bf16x3": Precision(F32, F32E),
    "fp32_bf16x3_6p": Precision(F32, F32E6),
}
PRECISIONS = tuple(TABLE)


def record(precision):
    """A precision name or a record -> the record; an unknown name raises ValueError."""
    if isinstance(precision, Precision):
        return precision
    if precision not in PRECISIONS:
        raise ValueError(precision)
    return TABLE[precision]
