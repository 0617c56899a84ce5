// Fused HiFi-GAN single-conv dilation unit, f32 operands (exact-f32 MFMA, v_mfma_f32_32x32x2_f32).
//
// The windows are the two-conv unit's (resunit_f32.hip); without the h tile a window stores all its columns, so what the tile choice trades is only
// workgroups per CU against the halo rows staged twice.  The V3 dilations reach (k - 1) dil = 72 rows: where the wide window no longer fits the
// 160 KiB beside them, the narrow one runs as one workgroup per CU.
#include "resunit1_impl.h"

int jatts_resunit1_f32(const jatts_resunit_desc& d, hipStream_t s) {
  const int halo = (d.k_w - 1) * d.dil;   // x-tile rows beyond the workgroup's columns
  // last template argument: residual kept in registers (x fetched once)
  switch (d.channels) {
    case 32:
      return launch_resunit1<float, 32, 512, 1, 4, 8, 2, true>(d, s);
    case 64:
      return launch_resunit1<float, 64, 256, 1, 2, 8, 2, true>(d, s);
    case 128:
      // 128 columns (4 waves): two workgroups per CU while the tile fits twice in 160 KiB; else 256 columns (8 waves), one per CU; past
      // that window's LDS (halo > 53 rows) the 128-column tile again, one per CU
      if (resunit1_lds<float, 128, 128>(halo) <= 80 * 1024 || resunit1_lds<float, 128, 256>(halo) > 160 * 1024)
        return d.k_w <= 7 ? launch_resunit1<float, 128, 128, 2, 2, 8, 2, true>(d, s) : launch_resunit1<float, 128, 128, 2, 2, 8, 2>(d, s);
      return launch_resunit1<float, 128, 256, 2, 2, 8, 2>(d, s);
    case 256:
      if (resunit1_lds<float, 256, 128>(halo) <= 160 * 1024) return launch_resunit1<float, 256, 128, 4, 4, 8, 1>(d, s);
      return launch_resunit1<float, 256, 96, 4, 3, 8, 1, true>(d, s);
  }
  return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "resunit (single conv): unsupported channels for JATTS_F32 (32 / 64 / 128 / 256)");
}
