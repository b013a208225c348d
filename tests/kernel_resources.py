"""Register and scratch figures of the kernels of one HIP source, from the compiler's own resource remarks."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resource_usage(src, out_name, device_only=False):
    """{kernel symbol: {"VGPRs", "AGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]"}} of one compilation of src for gfx950."""
    from gp_amd import _build
    out = os.path.join(ROOT, "build", "resource_check")
    os.makedirs(out, exist_ok=True)
    cmd = [_build.hipcc(), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++20", "-fPIC", "-c", src, "-o",
           os.path.join(out, out_name), "-Rpass-analysis=kernel-resource-usage"] + (["--cuda-device-only"] if device_only else [])
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=_build.CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        mm = re.search(r"Function Name: (\S+)", line)
        if mm:
            name = mm.group(1); kernels[name] = {}
            continue
        mm = re.search(r"remark:\s+(VGPRs Spill|VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if mm and name:
            kernels[name][mm.group(1)] = int(mm.group(2))
    return kernels
