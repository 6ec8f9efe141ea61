#!/bin/bash
cd /tmp && export TMPDIR=/tmp
R=/root/repo
KDB_HOST_CHUNK_MIN=0 python $R/scripts/pcie_probe.py 2>&1 | grep -E "B=|KDB|sig"
python $R/scripts/pcie_probe.py 2>&1 | grep -E "B=|KDB|sig"
