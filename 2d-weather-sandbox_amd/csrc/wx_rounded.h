// wx_rounded.h -- `rounded`: a product that feeds a sum or a difference is a value of its own. The contraction pragma at the head of
// a function that rounds is what says so to the compiler's front end; a device build with -ffp-contract=fast (libwxsim_fast.so) also
// lets the code generator fuse ANY multiply with a dependent add, pragma or not, so on the device the product additionally passes
// through an empty statement the code generator cannot look through: it is rounded to double before the sum sees it, in every build.
// Plain C++ that a host compiler takes without the HIP headers (there it is the identity). Shared by the per-cell functions of the
// ensemble calls: wx_ens_perturb_cell.h, wx_ens_quant_cell.h, wx_ens_stat.h, wx_ens_assim_cell.h. (WX_HD: wx_ens_cell_common.h.)
#pragma once
#include "wx_ens_cell_common.h"

namespace wxr {

WX_HD inline double rounded(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(x));
#endif
  return x;
}

} // namespace wxr
