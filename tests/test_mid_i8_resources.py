"""k_mid_eval_i8 (csrc/mid_i8.h) holds its 512-row train tile in registers and sits at the 256-VGPR ceiling of two waves per SIMD: an edit
or a compiler that pushes it over would spill into scratch without a word and the sweep would crawl.  No GPU here: match.hip is compiled
for gfx950 with the compiler's resource report, and the kernel must show no scratch, no spill and two waves per SIMD."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_the_mfma_sweep_keeps_its_tile_in_registers(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-Wno-pass-failed",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "reconstructor_amd", "csrc", "match.hip"),
                        "-o", str(tmp_path / "match.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if "Function Name: _Z13k_mid_eval_i87MidArgs" in ln]
    assert len(at) == 1, "k_mid_eval_i8 is not in the resource report"
    rep = {}
    for ln in lines[at[0] + 1:at[0] + 16]:        # (the report of one kernel: its lines follow the name, behind the quoted source line)
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\w+) \[-Rpass", ln)
        if m and m.group(1).strip() == "Function Name":
            break                                     # the next kernel's report
        if m:
            rep[m.group(1).strip()] = m.group(2)
    print(rep)
    assert rep["ScratchSize [bytes/lane]"] == "0" and rep["VGPRs Spill"] == "0" and rep["SGPRs Spill"] == "0", rep
    assert int(rep["VGPRs"]) + int(rep["AGPRs"]) <= 256 and rep["Occupancy [waves/SIMD]"] == "2", rep
