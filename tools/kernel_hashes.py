#!/usr/bin/env python3
"""One line `sha1 symbol` per GPU kernel in device assembly (hipcc HIPFLAGS --cuda-device-only -S), sorted by symbol:
diff the lists of two source trees to see that a host-side change left every kernel's instructions and .amdhsa_kernel
block alone.  Local label numbers (they count functions and blocks in file order) are normalised, comments dropped.

    for f in iac_amd/csrc/*.hip; do hipcc $HIPFLAGS --cuda-device-only -S $f -o out/$(basename $f).s; done
    tools/kernel_hashes.py out/*.s > kernels.txt

--anon hashes each body with the kernel's own symbol replaced by a fixed token, so that a kernel that was only renamed
(a template argument added, two templates folded into one) keeps its hash and can be paired with the other tree's.
"""
import hashlib
import re
import sys

BODY = re.compile(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", re.M | re.S)
LOCAL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+")
COMMENT = re.compile(r"\s*;.*$", re.M)

args = sys.argv[1:]
anon = "--anon" in args
rows = []
for path in (a for a in args if a != "--anon"):
    for sym, body in BODY.findall(open(path).read()):
        if ".amdhsa_kernel " + sym + "\n" in body:   # kernels only: device functions have no descriptor
            if anon:
                body = body.replace(sym, "@KERNEL@")
            rows.append((sym, hashlib.sha1(LOCAL.sub(r".\1", COMMENT.sub("", body)).encode()).hexdigest()))
for sym, h in sorted(rows):
    print(h, sym)
