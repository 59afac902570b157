#!/usr/bin/env python3
"""SHA-256 of the gfx950 machine code (.text of the device ELF) inside compiled objects of fit-slam_amd/csrc — what "the tuned
kernels' machine code is byte for byte the parent's" is shown with.  The fat binary as a whole is no good for that: it carries a
compilation-unit id derived from the source file's path, so two checkouts never agree on it.

    python tools/code_object_digest.py                       # this tree's objects (build first)
    python tools/code_object_digest.py --against OTHER_TREE  # ... beside another tree's, with a verdict per file
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMED = ["fs_fim", "fs_raymarch", "fs_rank", "fs_sort", "fs_gridops"]


def _llvm(tool):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/lib/llvm/bin", os.path.dirname(shutil.which("hipcc") or "")):
        p = os.path.join(d, tool)
        if os.path.exists(p):
            return p
    raise SystemExit(f"{tool} not found")


def text_digest(obj):
    with tempfile.TemporaryDirectory() as tmp:
        fat, co, text = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "device.co"), os.path.join(tmp, "text.bin")
        subprocess.run([_llvm("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([_llvm("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}",
                        f"--output={co}", "--unbundle"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        subprocess.run([_llvm("llvm-objcopy"), "-O", "binary", "--only-section=.text", co, text], check=True)
        data = open(text, "rb").read()
    return hashlib.sha256(data).hexdigest(), len(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", help="another checkout (built) to compare with")
    ap.add_argument("--files", nargs="*", default=TIMED)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows, same = {}, True
    for name in a.files:
        here = text_digest(os.path.join(ROOT, "fit-slam_amd", "csrc", name + ".o"))
        row = {"sha256": here[0], "text_bytes": here[1]}
        if a.against:
            there = text_digest(os.path.join(a.against, "fit-slam_amd", "csrc", name + ".o"))
            row.update(other_sha256=there[0], other_text_bytes=there[1], identical=here == there)
            same = same and here == there
        rows[name + ".hip"] = row
    text = json.dumps(rows, indent=1, sort_keys=True)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
