#!/bin/bash
# The compiler's resource report and the code size of kernels (no GPU needed).
#   bash tools/resource_usage.sh > profiles/r06_resource_usage.txt                       # the 4-SPS burst kernels
#   bash tools/resource_usage.sh trx_tx_frontend.hip 'synthesis|tx_' > profiles/tx_frontend_resource_usage.txt
# Arguments: a source file of osmo_trx_amd/csrc/ and an extended regular expression that selects kernels by name.
R=$(cd "$(dirname "$0")/.." && pwd)
SRC=${1:-trx_kernel4.hip}
PAT=${2:-pull4}
T=$(mktemp -d)
echo "# hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage osmo_trx_amd/csrc/$SRC (the tree of this commit; tools/resource_usage.sh)"
if [ "$SRC" = trx_kernel4.hip ]; then
	echo "# nb_pull4_kernel = the normal-burst kernel; burst_pull4_kernel<false,false,true,LIST> = the general kernel's common instantiation (LIST: behind the normal-burst kernel)"
fi
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -w -I$R/include -c --cuda-device-only --no-gpu-bundle-output \
	-Rpass-analysis=kernel-resource-usage -o $T/k.o $R/osmo_trx_amd/csrc/$SRC 2>&1 |
	grep "remark:" | sed 's/.*remark: //; s/ \[-Rpass-analysis=kernel-resource-usage\]//' | grep -v "^\s*$" |
	awk -v pat="$PAT" '/Function Name/{on = ($0 ~ pat)} on{print}'
echo
echo "# code size (llvm-readelf -s, bytes):"
/opt/rocm/lib/llvm/bin/llvm-readelf -s $T/k.o | awk -v pat="$PAT" '$4 == "FUNC" && $8 ~ pat && !seen[$8]++ {print $3, $8}'
rm -rf $T
