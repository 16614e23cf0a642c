#!/bin/bash
# disassemble one kernel of one of libqbhip's kernel objects: tools/lab/isa.sh <source stem> '<mangled-name regex>' > out.s
# (e.g. tools/lab/isa.sh qbh_spmv_wave '_ZN3qbh12k_spmv_wave2ILi2ELi2ELb1ELb1EEEvNS_8SpmvArgsE')
set -e
D=$(mktemp -d)
cp "$(cd "$(dirname "$0")/../.." && pwd)/quantum_basis_amd/csrc/build/$1.hip.o" $D/k.o
(cd $D && /opt/rocm/lib/llvm/bin/llvm-objdump -d --offloading k.o > /dev/null 2>&1 || true)
/opt/rocm/lib/llvm/bin/llvm-objdump -d $D/k.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 | awk -v pat="$2" '$0 ~ "^[0-9a-f]+ <" pat ">:" {p=1} p&&/s_endpgm/{print; exit} p{print}'
rm -rf $D
