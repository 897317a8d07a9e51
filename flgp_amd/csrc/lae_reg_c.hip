// Register-resident LAE, r = 11..16 (d <= 32) -- see lae_reg.h.
#include "lae_reg.h"

namespace flgp {
int launch_lae_reg_hi(FLGP_LAE_REG_ARGS, int r) {
  switch (r) {
    case 11: return launch_lae_reg_r<11>(FLGP_LAE_REG_PASS);
    case 12: return launch_lae_reg_r<12>(FLGP_LAE_REG_PASS);
    case 13: return launch_lae_reg_r<13>(FLGP_LAE_REG_PASS);
    case 14: return launch_lae_reg_r<14>(FLGP_LAE_REG_PASS);
    case 15: return launch_lae_reg_r<15>(FLGP_LAE_REG_PASS);
    case 16: return launch_lae_reg_r<16>(FLGP_LAE_REG_PASS);
  }
  return FLGP_LAE_REG_NONE;
}
}  // namespace flgp
