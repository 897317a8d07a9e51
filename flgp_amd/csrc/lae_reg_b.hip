// Register-resident LAE, r = 2..9 -- see lae_reg.h.
#include "lae_reg.h"

namespace flgp {
int launch_lae_reg_lo(FLGP_LAE_REG_ARGS, int r) {
  switch (r) {
    case 2: return launch_lae_reg_r<2>(FLGP_LAE_REG_PASS);
    case 3: return launch_lae_reg_r<3>(FLGP_LAE_REG_PASS);
    case 4: return launch_lae_reg_r<4>(FLGP_LAE_REG_PASS);
    case 5: return launch_lae_reg_r<5>(FLGP_LAE_REG_PASS);
    case 6: return launch_lae_reg_r<6>(FLGP_LAE_REG_PASS);
    case 7: return launch_lae_reg_r<7>(FLGP_LAE_REG_PASS);
    case 8: return launch_lae_reg_r<8>(FLGP_LAE_REG_PASS);
    case 9: return launch_lae_reg_r<9>(FLGP_LAE_REG_PASS);
  }
  return FLGP_LAE_REG_NONE;
}
}  // namespace flgp
