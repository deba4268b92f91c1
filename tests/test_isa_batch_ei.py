"""The analytic batch EI's kernels must compile for gfx950 without scratch (CPU test: hipcc cross-compiles).

Why it is a test: the forward tail's chain already holds ~190 live doubles at QP = 16 (215 VGPRs), and the gradient tail
that now shares its file keeps the chain's intermediates for the reverse pass on top.  The forward tail must not pay for
its new neighbour, and the gradient tail's sample loops must stay free of scratch accesses (at QP = 16 it reduces the
factor's adjoint over the wave per 64-sample chunk precisely so that no per-lane accumulators are needed): a source
change that brings spills into those loops is a performance regression no parity test sees."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _kernels(tmp_path):
    src = os.path.join(ROOT, "trieste_amd", "csrc", "tgp_kernels_bei.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-save-temps", "-c", src, "-o", "bei.o"],
                   cwd=tmp_path, check=True, capture_output=True, timeout=900)
    (asm,) = glob.glob(os.path.join(tmp_path, "*gfx950.s"))
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".end_amdhsa_kernel")]
        depth, per_depth = 0, {}
        for line in body.splitlines():
            if line.startswith(".LBB") or line.startswith("; %bb"):
                m = re.search(r"Depth=(\d+)", line)
                depth = int(m.group(1)) if m else 0
            if "scratch_" in line:
                per_depth[depth] = per_depth.get(depth, 0) + 1
        field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", block).group(1))  # noqa: E731
        out[name] = {"vgprs": field("vgpr_count"), "agprs": int(block.split()[0]),
                     "scratch_bytes": field("private_segment_fixed_size"), "scratch_per_depth": per_depth,
                     "lds_static": field("group_segment_fixed_size")}
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_batch_ei_kernels_use_no_scratch(tmp_path):
    kernels = _kernels(tmp_path)
    fwd = {n: k for n, k in kernels.items() if "bei_tail_kernel" in n}
    grad = {n: k for n, k in kernels.items() if "bei_grad_tail_kernel" in n}
    assert len(fwd) == 3 and len(grad) == 3, sorted(kernels)
    for n, k in sorted(kernels.items()):
        # vgprs is the unified count (architectural + accumulation registers); a 256-thread workgroup may hold 512 per lane
        print(f"{n}: {k['vgprs']} VGPRs (of them {k['agprs']} AGPRs), {k['scratch_bytes']} bytes of scratch, "
              f"scratch accesses per loop depth {k['scratch_per_depth']}")
    for n, k in fwd.items():
        assert k["scratch_bytes"] == 0 and not k["scratch_per_depth"], f"{n}: the forward tail spills: {k}"
        assert k["vgprs"] <= 256, f"{n}: the forward tail no longer fits two workgroups per CU: {k}"
    for n, k in grad.items():
        assert k["scratch_bytes"] == 0 and not k["scratch_per_depth"], f"{n}: the gradient tail spills to scratch: {k}"
        assert k["vgprs"] <= 512, n
