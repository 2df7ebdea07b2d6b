#!/usr/bin/env python3
"""sha256 of every device function's machine code in a compiled HIP object, and the difference
between two builds: the evidence that a change left existing kernels' code alone.

    python tools/device_text_hashes.py build/sdl/pipeline.hip.o                 # name -> hash
    python tools/device_text_hashes.py OLD.o NEW.o                              # what differs

The gfx950 code object is unbundled from the host object's .hip_fatbin section
(llvm-objcopy, clang-offload-bundler), its symbol
table read with llvm-readelf and the functions' bytes cut out of .text.  Exit status 1 when a
function present in both objects differs.
"""
import hashlib
import os
import subprocess
import sys
import tempfile

ROCM_LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
ARCH = os.environ.get("SDL_OFFLOAD_ARCH", "gfx950")


def tool(name):
    p = os.path.join(ROCM_LLVM, name)
    return p if os.path.exists(p) else name


def functions(obj):
    """{symbol: sha256 of its bytes} for the FUNC symbols of the object's device .text."""
    with tempfile.TemporaryDirectory() as tmp:
        co, fat = os.path.join(tmp, "device.co"), os.path.join(tmp, "fat.bin")
        subprocess.run([tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj], check=True)
        subprocess.run([tool("clang-offload-bundler"), "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}",
                        f"--input={fat}", f"--output={co}", "--unbundle"], check=True)
        text = os.path.join(tmp, "text.bin")
        subprocess.run([tool("llvm-objcopy"), "-O", "binary", "--only-section=.text", co, text], check=True)
        with open(text, "rb") as f:
            code = f.read()
        secs = subprocess.run([tool("llvm-readelf"), "-S", "-W", co], check=True, capture_output=True, text=True).stdout
        base = None
        for line in secs.splitlines():
            parts = line.replace("[", " ").replace("]", " ").split()
            if len(parts) > 3 and parts[1] == ".text":
                base = int(parts[3], 16)
        syms = subprocess.run([tool("llvm-readelf"), "-s", "-W", co], check=True, capture_output=True, text=True).stdout
        out = {}
        for line in syms.splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] == "FUNC" and p[6] != "UND":
                addr, size = int(p[1], 16) - base, int(p[2])
                out[p[7]] = hashlib.sha256(code[addr:addr + size]).hexdigest()
        return out


def main(argv):
    if len(argv) == 2:
        for name, h in sorted(functions(argv[1]).items()):
            print(h, name)
        return 0
    old, new = functions(argv[1]), functions(argv[2])
    changed = sorted(n for n in old if n in new and old[n] != new[n])
    print(f"{len(old)} functions before, {len(new)} after, {len(set(old) & set(new))} in both, "
          f"{len(changed)} of those differ")
    for n in sorted(set(new) - set(old)):
        print("added  ", n)
    for n in sorted(set(old) - set(new)):
        print("removed", n)
    for n in changed:
        print("differs", n)
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    sys.exit(main(sys.argv))
