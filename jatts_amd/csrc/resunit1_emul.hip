// Fused HiFi-GAN single-conv dilation unit, f32 activations in HBM, f32-EQUIVALENT emulated MFMA operands (three bf16 terms per value): JATTS_F32E (seven
// partial products per product) and JATTS_F32E6 (six), on v_mfma_f32_16x16x32_bf16 (w_layout = 1 weights; resunit1_emul16_impl.h).
//
// The windows are the two-conv unit's (resunit_emul.hip: resunit_emul16).  The w_layout = 0 (32 x 32 x 16) form has no single-conv kernel: no generator
// packs these units that way.
#include "resunit1_emul16_impl.h"

template <typename T>
static int resunit1_emul16(const jatts_resunit_desc& d, hipStream_t s) {
  const int halo = (d.k_w - 1) * d.dil;
  switch (d.channels) {
    // C <= 64: the residual from registers (RREG)
    case 32: return launch_resunit1_emul16<T, 32, 256, 1, 4, 2, false, true>(d, s);
    case 64:
      if (d.k_w >= 11) return launch_resunit1_emul16<T, 64, 256, 1, 4, 1, false, true>(d, s);
      return launch_resunit1_emul16<T, 64, 128, 2, 2, 2, false, true>(d, s);
    case 128: return launch_resunit1_emul16<T, 128, 128, 2, 2, 1>(d, s);
    case 256:
      // the one-piece x tile where it fits; k = 11, dilation 5: the 114-row x tile one channel half at a time
      if (resunit1_emul16_region<256, 64>(halo) + 1024 <= 160 * 1024) return launch_resunit1_emul16<T, 256, 64, 4, 1, 1>(d, s);
      return launch_resunit1_emul16<T, 256, 64, 4, 1, 1, true>(d, s);
  }
  return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "resunit (single conv): unsupported channels for JATTS_F32E (32 / 64 / 128 / 256)");
}

int jatts_resunit1_emul(const jatts_resunit_desc& d, hipStream_t s) {
  if (d.w_layout != 1)
    return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "resunit (single conv): JATTS_F32E / JATTS_F32E6 take w_layout = 1 weights only (pack_unit_weight_bf16x3_k32)");
  return d.dtype == JATTS_F32E6 ? resunit1_emul16<bf3f>(d, s) : resunit1_emul16<bf3>(d, s);
}
