#!/bin/bash
# kernel resource usage of one csrc file as the Makefile builds it:  tools/kres.sh mrgs_render_fwd.hip [extra flags]
# prints name / VGPRs / scratch / occupancy / spills / LDS per kernel
cd "$(dirname "$0")/../materialrefgs_amd/csrc" || exit 1
f=$1; shift
# the compile line is the Makefile's own (a dry run of the object rule): the flag table lives there and nowhere else
line=$(make -n -B "${f%.hip}.o" | grep -- "-c $f") || exit 1
${line% -o *} "$@" -Rpass-analysis=kernel-resource-usage -o /tmp/kres_$$.o 2>&1 | \
  grep -E "Function Name|VGPRs:|VGPRs Spill|ScratchSize|Occupancy|LDS Size" | \
  sed -E 's/.*remark: +//; s/ \[-Rpass.*//' | paste - - - - - - | \
  sed -E 's/Function Name: (_Z[0-9]+)?/ /' | awk '{n=$1; $1=""; printf "%-60.60s %s\n", n, $0}'
rm -f /tmp/kres_$$.o
