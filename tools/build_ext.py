#!/usr/bin/env python3
"""In-tree build of mpi4torch_amd/_C.so with explicit hipcc for gfx950.

No hipify, no CUDA shims: csrc/ is written directly against HIP/RCCL and
the torch-ROCm headers. The built .so lands inside the package so it travels
with repo snapshots (gpurun) and is found without installation.

Usage: python tools/build_ext.py [--force]
"""
import os
import subprocess
import sys
import sysconfig

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "csrc")
BUILD = os.path.join(REPO, "build")
OUT = os.path.join(REPO, "mpi4torch_amd", "_C.so")

SOURCES = [
    "kernels.hip",
    "mx8_kernels.hip",
    "transport.cpp",
    "ops.cpp",
    "extension.cpp",
]

HEADERS = ["common.hpp", "kernels.hpp", "transport.hpp", "ops.hpp"]

GPU_ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def torch_paths():
    import torch

    t = os.path.dirname(torch.__file__)
    return t


def build(force: bool = False, verbose: bool = True) -> str:
    t = torch_paths()
    os.makedirs(BUILD, exist_ok=True)

    includes = [
        os.path.join(t, "include"),
        os.path.join(t, "include", "torch", "csrc", "api", "include"),
        sysconfig.get_paths()["include"],
        "/opt/rocm/include",
    ]
    common_flags = (
        [f"-I{i}" for i in includes]
        + [
            "-D__HIP_PLATFORM_AMD__=1",
            "-DUSE_ROCM=1",
            "-DHIPBLAS_V2",
            "-D_GLIBCXX_USE_CXX11_ABI=1",
            "-DTORCH_EXTENSION_NAME=_C",
            "-fPIC",
            "-std=c++17",
            "-O3",
        ]
    )

    objs = []
    hdr_mtime = max(
        os.path.getmtime(os.path.join(CSRC, h)) for h in HEADERS
    )
    self_mtime = os.path.getmtime(os.path.abspath(__file__))
    jobs = []
    for src in SOURCES:
        spath = os.path.join(CSRC, src)
        obj = os.path.join(BUILD, src.replace("/", "_") + ".o")
        objs.append(obj)
        if (
            not force
            and os.path.exists(obj)
            and os.path.getmtime(obj) > os.path.getmtime(spath)
            and os.path.getmtime(obj) > hdr_mtime
            and os.path.getmtime(obj) > self_mtime
        ):
            continue
        cmd = ["hipcc", "-c", spath, "-o", obj] + common_flags
        # hipcc compiles every TU in hip mode; pin the device pass to the
        # real target so host-only files are not cross-checked for gfx906
        cmd.append(f"--offload-arch={GPU_ARCH}")
        if verbose:
            print("[build_ext]", " ".join(cmd), flush=True)
        jobs.append(subprocess.Popen(cmd, cwd=REPO))
    failed = [j.wait() for j in jobs]  # TUs are independent: compile parallel
    if any(failed):
        raise RuntimeError("hipcc compilation failed")

    if (
        force
        or not os.path.exists(OUT)
        or any(os.path.getmtime(o) > os.path.getmtime(OUT) for o in objs)
    ):
        link = (
            ["hipcc", "-shared", "-o", OUT]
            + objs
            + [
                f"-L{os.path.join(t, 'lib')}",
                "-ltorch",
                "-ltorch_cpu",
                "-ltorch_python",
                "-ltorch_hip",
                "-lc10",
                "-lc10_hip",
                "-lrccl",
                "-lamdhip64",
                f"-Wl,-rpath,{os.path.join(t, 'lib')}",
                "-Wl,-rpath,/opt/rocm/lib",
            ]
        )
        if verbose:
            print("[build_ext]", " ".join(link), flush=True)
        subprocess.check_call(link, cwd=REPO)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print("built", OUT)
