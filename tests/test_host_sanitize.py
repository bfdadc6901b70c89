"""SURVEY section 5 (race / memory checking): GPU AddressSanitizer is not available on this pool, so the HOST half of the C-ABI
library - parameter store, validation, LayerNorm / FiLM folding, weight packing into the arena, the music encoder's BatchNorm
folding and its stem / conv / conv4 / proj packers (csrc/dc_pack.h), schedule and filter tables - is built with AddressSanitizer + UBSan on the host side only (-Xarch_host on the compile, -fno-gpu-sanitize on the link;
-DDC_HOST_SANITIZE: a sampler can be created without a device) and driven through its entry points by tests/san_child.py, run
by a Python launcher that carries the sanitizer runtime itself (linked statically), in a process with no device visible."""
import os
import shutil
import subprocess
import sys
import sysconfig

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffusion-conductor_amd")


def test_host_half_under_address_and_ub_sanitizers():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    clangxx = "/opt/rocm/lib/llvm/bin/clang++"
    rt = subprocess.run([clangxx, "-print-file-name=libclang_rt.asan-x86_64.a"], capture_output=True, text=True).stdout.strip()
    if not os.path.exists(rt):
        pytest.skip("no ASan runtime in this toolchain")
    sys.path.insert(0, ROOT)
    from diffusion_conductor_amd import native
    native.build_library()                         # the other translation units' objects (device code: not instrumented)
    bdir = os.path.join(PKG, "build", "san")
    os.makedirs(bdir, exist_ok=True)
    obj, so = os.path.join(bdir, "dc_api_san.o"), os.path.join(bdir, "libdc_ddim_san.alt")
    launcher = os.path.join(bdir, "python_san")
    src = os.path.join(PKG, "csrc", "dc_api.hip")
    deps = [src] + [os.path.join(PKG, "csrc", h) for h in native.HEADERS] + [os.path.join(ROOT, "include", "dc_ddim.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wno-unused-value",
                        "-DDC_HOST_SANITIZE", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        "-Xarch_host", "-fno-omit-frame-pointer", "-c", src, "-o", obj], check=True)
        others = [os.path.join(PKG, "build", f.replace(".hip", ".o")) for f in native.SOURCES if f != "dc_api.hip"]
        # the sanitizer runtime is not linked into the library: it binds to the launcher's copy when loaded
        subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fno-gpu-sanitize", "-fsanitize=address,undefined", obj,
                        *others, "-o", so], check=True)
    if not os.path.exists(launcher):
        # a Python interpreter whose executable carries the ASan + UBSan runtime, so the instrumented library finds it in place
        inc = sysconfig.get_paths()["include"]
        libdir, ver = sysconfig.get_config_var("LIBDIR"), sysconfig.get_config_var("LDVERSION")
        main_c = os.path.join(bdir, "python_san.cpp")
        with open(main_c, "w") as f:
            f.write("#include <Python.h>\nint main(int argc, char** argv) { return Py_BytesMain(argc, argv); }\n")
        subprocess.run([clangxx, "-O1", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-I", inc, main_c, "-L", libdir,
                        f"-lpython{ver}", f"-Wl,-rpath,{libdir}", "-o", launcher], check=True)
    env = dict(os.environ, DC_DDIM_LIB=so, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ROCR_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="",
               PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([launcher, os.path.join(ROOT, "tests", "san_child.py")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "host sanitize pass: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
