#!/usr/bin/env python3
"""tools/mfma_error_stress.py <out.json> -- the coarse pass's error bound ON THE HARDWARE, on inputs that reach it.

tools/mfma_error_model.py measures |MFMA accumulator - exact value| / eps(q) on five benign data sets, where rounding errors cancel
and the largest excursion is a tenth of the bound.  This script points the same instrument (`measure`: the diagnostic build's packed
(best, second) table against float64 accumulators) at the sets of tests/coarse_stress.py, for D = 32, 40, 64, 100, 128, 256:
    aligned             every product of a query and its twin errs in the same direction: the first term of eps is nearly met
    accumulation-only   fp16-exact operands: what is left is the MFMA's accumulation and the fp32 half-norm, judged against eps_acc
    misranked           the coarse pass's second candidate is not the second neighbour
and asserts, per set and D:  excursion <= 1 and shortfall <= 1 (`measure`: the bound itself); the aligned set reaches the
emulation's value less 0.1 (otherwise the run did not exercise what it claims to); the table after upload (k_prepare) and after
upload_batch (k_prepare_batch: a second copy of the conversion) are byte-equal; at least one misranked second shows in the device's
own table.  The kernel form is whatever the diagnostic build's switches select (RCN_COARSE_S16 = 0 / 1, RCN_COARSE_W4 = 1): the
JSON names it.  Run with RCN_LIB=tools/librcn_diag.so (tests/test_coarse_stress_gpu.py does);  --all <out.json> runs every form in a
child process of its own and writes one file (profiles/mfma_error_stress.json)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import coarse_stress as cs  # noqa: E402
import mfma_error_model as mem  # noqa: E402  (sets RCN_COARSE_I8=0: 256-d rows stay on the fp16 kernel)


def run_set(m, lib, name, g, D):
    """One set (several pairs) at one D: `measure` per pair through both ingestion paths, folded into one entry."""
    entry = {"D": D, "excursion_in_eps": 0.0, "most_positive_excursion_in_eps": 0.0, "most_negative_excursion_in_eps": 0.0,
             "non_candidate_shortfall_in_eps": 0.0, "emulated_excursion_in_eps": 0.0, "misranked_seconds_in_device_table": 0, "rows": 0}
    if name == "accumulation_only":
        entry.update({"excursion_in_eps_acc": 0.0, "emulated_excursion_in_eps_acc": 0.0, "best_candidate_quantum_in_eps_acc_smallest": np.inf})
    for (a, b) in g["pairs"]:
        q, t = g["images"][a], g["images"][b]
        res, det = mem.measure(m, lib, q, t, detail=True)
        _, det_b = mem.measure(m, lib, q, t, detail=True, batch=True)
        assert det["cand"].tobytes() == det_b["cand"].tobytes(), (name, D, "k_prepare and k_prepare_batch leave different candidate tables")
        mdl = det["model"]
        ref = cs.model([q, t], D)
        assert all(mdl[k] == ref[k] for k in ("s", "bias", "nmax", "DP")), (name, D, mdl, ref)
        assert np.allclose(cs.eps(ref, cs.qnorm(q)), det["eps"], rtol=1e-12, atol=0)      # the tool's copy of the formula and the tests' copy
        acc, exact = cs.emulate(q, t, ref)
        entry["emulated_excursion_in_eps"] = max(entry["emulated_excursion_in_eps"], float((np.abs(acc - exact) / det["eps"][:, None]).max()))
        sg = det["signed_excursion_in_eps"]
        w = int(np.abs(sg).argmax())
        if np.abs(sg[w]) >= entry["excursion_in_eps"]:
            entry["worst_pair_query_row"] = [int(a), w, int(det["row"][w])]
            entry["best_candidate_quantum_in_eps_at_worst_query"] = float((det["hi"][w, 0] - det["lo"][w, 0]) / det["eps"][w])
        entry["excursion_in_eps"] = max(entry["excursion_in_eps"], res["candidate_excess_over_quantisation_interval_in_eps"])
        assert entry["excursion_in_eps"] >= float(np.abs(sg).max())
        entry["most_positive_excursion_in_eps"] = max(entry["most_positive_excursion_in_eps"], float(sg.max()))
        entry["most_negative_excursion_in_eps"] = min(entry["most_negative_excursion_in_eps"], float(sg.min()))
        entry["non_candidate_shortfall_in_eps"] = max(entry["non_candidate_shortfall_in_eps"], res["non_candidate_shortfall_in_eps"])
        if name == "accumulation_only":
            ea = cs.eps_acc(ref, cs.qnorm(q))
            entry["excursion_in_eps_acc"] = max(entry["excursion_in_eps_acc"], float((np.abs(sg) * det["eps"] / ea).max()))
            entry["emulated_excursion_in_eps_acc"] = max(entry["emulated_excursion_in_eps_acc"], float((np.abs(acc - exact) / ea[:, None]).max()))
            entry["best_candidate_quantum_in_eps_acc_smallest"] = min(entry["best_candidate_quantum_in_eps_acc_smallest"],
                                                                      float(((det["hi"][:, 0] - det["lo"][:, 0]) / ea).min()))
        # the second candidate of the device's table against the exact second neighbour (float64 accumulators order like distances)
        second = np.argsort(det["exact"], axis=1, kind="stable")[:, 1]
        entry["misranked_seconds_in_device_table"] += int((det["idx"][:, 1] != second).sum())
        entry["rows"] += len(q)
        entry["DP"] = res["DP"]
        entry["scale_log2"] = res["scale_log2"]
    entry["kernel_form"] = mem.kernel_form(entry["DP"])
    assert entry["excursion_in_eps"] <= 1.0 and entry["non_candidate_shortfall_in_eps"] <= 1.0, (name, entry)
    if name == "aligned":
        # both ends: the down-type pair's accumulators lie above the exact values, the up-type pair's below
        reach = min(entry["most_positive_excursion_in_eps"], -entry["most_negative_excursion_in_eps"])
        assert reach >= entry["emulated_excursion_in_eps"] - 0.1, (name, D, "the run did not reach the bound it claims to exercise", entry)
    if name == "accumulation_only":
        assert entry["excursion_in_eps_acc"] <= 1.0, (name, entry)
    if name == "misranked":
        assert entry["misranked_seconds_in_device_table"] >= 1, (name, entry)
    return entry


FORMS = {"shipped shape per D": {}, "RCN_COARSE_S16=0": {"RCN_COARSE_S16": "0"}, "RCN_COARSE_S16=1": {"RCN_COARSE_S16": "1"},
         "RCN_COARSE_W4=1": {"RCN_COARSE_W4": "1"}}


def all_forms(out):
    """--all <out.json>: one child process per form of K1 (fresh processes, one at a time), their tables in one file."""
    import subprocess
    import tempfile
    res = {}
    for form, env in FORMS.items():
        with tempfile.TemporaryDirectory() as d:
            f = os.path.join(d, "form.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), f], env=dict(os.environ, **env), check=True, timeout=600)
            res[form] = json.load(open(f))
    json.dump(res, open(out, "w"), indent=1)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--all":
        return all_forms(sys.argv[2])
    import torch  # noqa: F401
    from reconstructor_amd import _lib
    from reconstructor_amd.matcher import HipL2Matcher
    lib = _lib.load()
    assert b"DIAGNOSTIC" in lib.rcn_version(), "run with RCN_LIB=tools/librcn_diag.so"
    lib.rcn_diag_coarse_table.restype = C.c_int
    lib.rcn_diag_coarse_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double)]
    m = HipL2Matcher(device=0)
    w4 = os.environ.get("RCN_COARSE_W4") == "1"
    res = {}
    for name, gen in (("aligned", cs.aligned), ("accumulation_only", cs.accumulation_only), ("misranked", cs.misranked)):
        for D in cs.DIMS:
            if w4 and cs.padded(D) < 64:
                continue                     # k_coarse_w4 has no DP = 32 form
            key = "%s D=%d" % (name, D)
            res[key] = run_set(m, lib, name, gen(D), D)
            print(key, json.dumps(res[key]), flush=True)
    m.ctx.close()
    res["_note"] = ("units of eps(q) (accumulation_only also in eps_acc, the last three terms of eps): 0 = the exact accumulator lies inside "
                    "the truncated candidate's quantisation interval, 1 = at the certified bound; signed: + the accumulator lies above the exact "
                    "value; emulated: tests/coarse_stress.py on numpy's fp32 accumulation")
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
