// fb_qnet_x.hip -- the extended scalar loss kernels (FB_ALGO_DOUBLE_PER's target, the Huber loss) as a code object of their own.
// fb_qnet.hip is compiled a second time up to the two loss bodies; under FB_QNET_X_TU it ends with loss_head_x_kernel / fc1_bwd2_x_kernel's
// instantiations and their launchers (fb_common.h) in place of everything behind them.  Why: fb_qnet.hip, at FB_QNET_X_TU.
#define FB_QNET_X_TU 1
#include "fb_qnet.hip"
