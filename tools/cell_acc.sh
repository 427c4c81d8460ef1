#!/bin/bash
# Where does a workgroup of the column-pair cell kernel spend its time?  Development build (-DGPRX_CELL_ACC) beside the product library.
cd $GRAFT_REPO_ROOT
mkdir -p tools/_lib
cp gpras_amd/libgprx.so tools/_lib/libgprx_keep.so; GPRX_EXTRA_FLAGS=-DGPRX_CELL_ACC python3 -m gpras_amd._build --stale > /dev/null && cp gpras_amd/libgprx.so tools/_lib/libgprx_cellacc.so && cp tools/_lib/libgprx_keep.so gpras_amd/libgprx.so || exit 1
for cfg in "1024 512" "512 512"; do python3 tools/cell_acc.py $cfg tools/_lib/libgprx_cellacc.so; done
