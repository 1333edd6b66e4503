#!/bin/bash
# Builds probe variants of the fused kernel with shifted MFMA hook positions (-DFC_GEN_SHIFT=<k>, hundredths of a hook:
# fc_rq_eval_plan.h) into tools/probe/build/libfc_shift<k>.so.
set -e
cd "$(dirname "$0")/../.."
for k in "$@"; do
  EXTRA="-DFC_GEN_SHIFT=$k" tools/probe/build_fused_variants.sh 16 > /dev/null
  mv tools/probe/build/libfc_abl16.so tools/probe/build/libfc_shift$k.so
  echo built shift $k
done
