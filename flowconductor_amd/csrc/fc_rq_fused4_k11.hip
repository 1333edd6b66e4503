// K = 11, linear tails: instance of the K-generic resident-weight fused kernel (fc_rq_fused4_body.h), listed in FC_F4_INSTANCES (fc_rq_fused4.hip).
#define FC_F4_K 11
#define FC_F4_TAILS 1
#define FC_F4_NAME k11
#include "fc_rq_fused4_body.h"
