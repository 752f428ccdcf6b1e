#!/usr/bin/env python3
"""Per-kernel disassembly digests of a libsmi_amd.so, and their comparison.

  isa_symbols.py LIB                 one line per device function: sha256 of its
                                     disassembly (addresses and encodings
                                     stripped; branches are pc-relative)
  isa_symbols.py PARENT_LIB NEW_LIB  every symbol of PARENT_LIB looked up in
                                     NEW_LIB: identical / changed / missing,
                                     then the symbols only NEW_LIB has

Used to show that a change leaves existing kernels' instruction streams alone
(profiles/source/plain_symbols.txt).  Needs ROCm's llvm tools; no GPU.
"""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--" + os.environ.get("SMI_OFFLOAD_ARCH", "gfx950")
MAGICS = (b"__CLANG_OFFLOAD_BUNDLE__", b"CCOB")


def code_objects(lib: str, tmp: str) -> list[str]:
    """The device code objects of every offload bundle in the library's .hip_fatbin section."""
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib,
                    os.path.join(tmp, "copy.so")], check=True)
    data = open(fat, "rb").read()
    starts = sorted({m.start() for magic in MAGICS for m in re.finditer(re.escape(magic), data)})
    out = []
    for i, s in enumerate(starts):
        piece = os.path.join(tmp, f"bundle{i}")
        with open(piece, "wb") as f:
            f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = os.path.join(tmp, f"co{i}")
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={piece}",
                            f"--targets={TARGET}", f"--output={co}"], capture_output=True)
        if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) > 0:
            out.append(co)
    return out


def digests(lib: str) -> dict[str, str]:
    syms: dict[str, str] = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
            name, h = None, None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    if name:
                        syms[name] = h.hexdigest()
                    name, h = m.group(1), hashlib.sha256()
                elif name and line.strip() and line.strip() != "...":      # ("...": alignment padding behind a function)
                    h.update(re.sub(r"^\s*[0-9a-f]+:\s*", "", line.split("//")[0]).strip().encode() + b"\n")
            if name:
                syms[name] = h.hexdigest()
    return syms


def main() -> int:
    if len(sys.argv) == 2:
        for k, v in sorted(digests(sys.argv[1]).items()):
            print(v[:16], k)
        return 0
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    old, new = digests(sys.argv[1]), digests(sys.argv[2])
    same = [k for k in old if new.get(k) == old[k]]
    changed = [k for k in old if k in new and new[k] != old[k]]
    missing = [k for k in old if k not in new]
    print(f"parent symbols {len(old)}: identical {len(same)}, changed {len(changed)}, missing {len(missing)}; "
          f"new symbols {len(set(new) - set(old))}")
    for tag, names in (("CHANGED", changed), ("MISSING", missing), ("NEW", sorted(set(new) - set(old))),
                       ("IDENTICAL", sorted(same))):
        for k in names:
            print(tag, (new.get(k) or old[k])[:16], k)
    return 1 if changed or missing else 0


if __name__ == "__main__":
    sys.exit(main())
