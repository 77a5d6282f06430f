#!/usr/bin/env python3
"""One line `sha1 symbol` per GPU kernel in device assembly (hipcc HIPFLAGS --cuda-device-only -S), sorted by symbol:
diff the lists of two source trees to see that a host-side change left every kernel's instructions and .amdhsa_kernel
block alone.  Local label numbers (they count functions and blocks in file order) are normalised, comments dropped.

    for f in iac_amd/csrc/*.hip; do hipcc $HIPFLAGS --cuda-device-only -S $f -o out/$(basename $f).s; done
    tools/kernel_hashes.py out/*.s > kernels.txt
"""
import hashlib
import re
import sys

BODY = re.compile(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", re.M | re.S)
LOCAL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+")
COMMENT = re.compile(r"\s*;.*$", re.M)

rows = []
for path in sys.argv[1:]:
    for sym, body in BODY.findall(open(path).read()):
        if ".amdhsa_kernel " + sym + "\n" in body:   # kernels only: device functions have no descriptor
            rows.append((sym, hashlib.sha1(LOCAL.sub(r".\1", COMMENT.sub("", body)).encode()).hexdigest()))
for sym, h in sorted(rows):
    print(h, sym)
