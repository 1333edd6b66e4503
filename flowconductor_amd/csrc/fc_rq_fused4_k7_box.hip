// K = 7, no tails (coupling.py:543-547): instance of the K-generic resident-weight fused kernel (fc_rq_fused4_body.h), listed in FC_F4_INSTANCES (fc_rq_fused4.hip).
#define FC_F4_K 7
#define FC_F4_TAILS 0
#define FC_F4_NAME k7_box
#include "fc_rq_fused4_body.h"
