// Fused HiFi-GAN single-conv dilation unit, f16 operands and activations, f32 accumulate (v_mfma_f32_32x32x16_f16): 32 .. 512 channels.
// The windows are the two-conv unit's (resunit_f16_narrow.hip, resunit_f16_wide.hip).
#include "resunit1_impl.h"

int jatts_resunit1_f16(const jatts_resunit_desc& d, hipStream_t s) {
  const int halo = (d.k_w - 1) * d.dil;
  // tiles: <C, workgroup columns, waves along n, 32-col fragments per wave, weight-ring depth>
  switch (d.channels) {
    case 32: return d.k_w > 7 ? launch_resunit1<f16, 32, 512, 1, 4, 2>(d, s) : launch_resunit1<f16, 32, 256, 1, 2>(d, s);
    case 64: return d.k_w > 3 ? launch_resunit1<f16, 64, 512, 1, 4, 4>(d, s) : launch_resunit1<f16, 64, 256, 1, 2>(d, s);
    case 128:
      // two workgroups per CU with the 256-column window while its tile fits twice in 160 KiB, else the 3-fragment tile
      if (resunit1_lds<f16, 128, 256>(halo) * 2 > 160 * 1024) return launch_resunit1<f16, 128, 192, 2, 3, 4>(d, s);
      return launch_resunit1<f16, 128, 256, 2, 4, 4>(d, s);
    case 256: return launch_resunit1<f16, 256, 128, 4, 4, 4>(d, s);
    case 512: return launch_resunit1<f16, 512, 32, 4, 1>(d, s);
  }
  return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "resunit (single conv): unsupported channels for JATTS_F16 (32 / 64 / 128 / 256 / 512)");
}
