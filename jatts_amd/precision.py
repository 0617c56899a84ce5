"""The precisions: one record per name, for inference (Precision) and for the trainers (TrainArithmetic).  Pure Python (dtype codes from
_abi; no GPU, no torch).

``tensors`` is the dtype code of the activations in HBM, ``operand`` the operand code of a `dtype=F32` conv call site (hip.f32_operand):
F32S = split f16 hi/lo MFMA operands (hip.SplitWeight), F32E / F32E6 = three exact bf16 terms per operand, seven / six partial products
(hip.EmulWeight).  Everything else that depends on a precision name derives from these two fields.

A trainer's arithmetic is the pair TrainArithmetic(operand, attention): the operand code of the forward and data-gradient convs of
autograd.Conv1dFunction, and the code autograd.BMM asks its routing rule about for the attention products."""
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


class TrainArithmetic(NamedTuple):
    operand: int        # forward and data-gradient convs: F32, F32S or F32E
    attention: int      # the attention products of autograd.BMM: F32, or F32E where emul_bgemm_wins routes them


_TRAIN_OPERANDS = {
    F32: "exact-f32 MFMA, the reference's arithmetic",
    F32S: "f32 tensors; the forward and data-gradient convs on split f16 hi / lo MFMA operands, everything else exact f32",
    F32E: "f32 tensors; the forward, data-gradient and weight-gradient convs on three exact bf16 terms per operand (seven partial products, "
          "f32-equivalent), everything else exact f32",
}
# the trainers' precisions -> which contractions leave exact f32: the f32-tensor precisions of TABLE without the six-product form
TRAIN_PRECISIONS = {name: _TRAIN_OPERANDS[p.operand] for name, p in TABLE.items() if p.tensors == F32 and p.operand != F32E6}
# the trainers' attention= : the arithmetic of autograd.BMM's products -- q k^T, q p^T, P v, the Gaussian-upsampling p_up @ hs (while
# autograd.MAS_OWN_KERNELS leaves it on BMM) and their gradients.  Independent of the precision.
TRAIN_ATTENTIONS = {
    "fp32": "exact-f32 MFMA (the default, also None)",
    "fp32_bf16x3": "three exact bf16 terms per operand, seven partial products, for the product shapes emul_bgemm_wins routes; exact f32 elsewhere",
}


def _accepted(table):
    return " or ".join(f"{k!r} ({v})" for k, v in table.items())


def train_arithmetic(precision="fp32", attention=None):
    """A trainer's (precision, attention) names -> its TrainArithmetic; a record is returned as is.  attention None means exact f32.  An unknown
    name raises ValueError listing every accepted one with what it does."""
    if isinstance(precision, TrainArithmetic):
        return precision
    if precision not in TRAIN_PRECISIONS:
        raise ValueError(f"trainer precision {precision!r}: " + _accepted(TRAIN_PRECISIONS))
    if attention is not None and attention not in TRAIN_ATTENTIONS:
        raise ValueError(f"trainer attention {attention!r}: None or " + _accepted(TRAIN_ATTENTIONS))
    return TrainArithmetic(TABLE[precision].operand, F32 if attention is None else TABLE[attention].operand)
