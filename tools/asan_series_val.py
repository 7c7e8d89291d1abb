"""Host AddressSanitizer check of include/windgnn_series_val.h as a STAND-ALONE program (CPU only; no GPU is needed or used).

Builds every csrc/*.hip with `-fsanitize=address -fno-gpu-sanitize` (host code instrumented, device code untouched), links
tools/asan_series_val_main.cpp -- a program with its own main() that drives every validation path of wgnn_series_val,
wgnn_val_init, wgnn_val_begin and wgnn_val_close on fake device pointers -- against those objects, and runs it.  The sanitizer's
runtime is linked into the program: nothing is preloaded and no interpreter loads the library.  Every call must come back
refused from the host; any report or unexpected status fails the check.

    python tools/asan_series_val.py          # exit code 0 = clean
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "windgnn_amd", "csrc")
OUT = os.path.join(ROOT, "build", "asan_val")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address", "-fno-gpu-sanitize"]


def main() -> int:
    os.makedirs(OUT, exist_ok=True)
    from windgnn_amd.build import SOURCES
    flags = ["-O1", "-g", "--offload-arch=gfx950", "-fPIC", "-std=c++17", *SAN, "-mllvm", "-amdgpu-mfma-vgpr-form"]
    jobs = [(src, os.path.join(OUT, src.replace(".hip", ".o")), [HIPCC, *flags, "-c", os.path.join(CSRC, src)]) for src in SOURCES]
    main_src = os.path.join(ROOT, "tools", "asan_series_val_main.cpp")
    jobs.append((main_src, os.path.join(OUT, "main.o"), [HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", *SAN[:1], "-c", main_src]))
    procs = [(src, subprocess.Popen(cmd + ["-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for src, obj, cmd in jobs]
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            print("hipcc (asan) failed on %s:\n%s" % (src, out))
            return 2
    exe = os.path.join(OUT, "asan_series_val")
    subprocess.run([HIPCC, "--offload-arch=gfx950", *SAN, *[obj for _, obj, _ in jobs], "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    if r.returncode != 0 or "AddressSanitizer" in r.stdout:
        return r.returncode or 1
    return 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.exit(main())
