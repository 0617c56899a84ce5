// Fused HiFi-GAN dilation unit, f16 operands, 32 / 64 channels (the HBM-bound late stages).
#include "resunit_impl.h"

int jatts_resunit_f16_narrow(const jatts_resunit_desc& d, hipStream_t s) {
  // tiles: <C, workgroup columns, waves along n, 32-col fragments per wave, weight-ring depth>
  switch (d.channels) {
    case 32: return d.k_w > 7 ? launch_resunit<f16, 32, 512, 1, 4, 2>(d, s) : launch_resunit<f16, 32, 256, 1, 2>(d, s);
    case 64: return d.k_w > 3 ? launch_resunit<f16, 64, 512, 1, 4, 4>(d, s) : launch_resunit<f16, 64, 256, 1, 2>(d, s);
  }
  return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "resunit: unsupported channels/dtype (use jatts_conv1d)");
}
