"""Writes tests/golden/launch_plans.json: the launch plans (or refusals) of k_gemv_quad, its XF forms and k_gemv_rows over a grid of shapes,
row-quad counts, modes and forced configurations.

    python tests/golden/make_launch_plans.py [--exe PROGRAM] [--out FILE]

PROGRAM answers the queries of tests/cpp/launch_plan_main.cc; without --exe that program is compiled (g++) from the tree.  The committed
file was recorded with a PROGRAM built around the selection code as it stood before tmac_launch_plan.cpp existed (quad_config, qlaunch_nr,
qlaunch_xf_nr, qlaunch_xf_cfg, rows_plan and launch_gemv_rows' waves-per-quad and grid rule inside tmac_quad.hip / tmac_rows.hip, the launch
replaced by a print of its template arguments, grid and LDS bytes); run on the tree, this script must reproduce it byte for byte
(tests/test_launch_plan_cpu.py).  One rule has changed since and the file was recorded again from the tree: a k_gemv_quad launch that
copies the workspace's LUT image (build_lut = 0) used to be refused for K > 12288 by the builder's limit of six tables per thread, which
kept K = 14336 from the split and host-pointer entry points; those 908 answers are plans now and every other answer is as it was.

The file: "axes" (named lists of values), "answers" (the distinct answer lines) and "cases": [query template, axis, answer index per value
of the axis] -- the query is the template with {} replaced by the value.
"""
import argparse
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# K: nst = 1, 2, 3, 4, 6 (2048, 4096, 6144, 8192, 12288), ragged 3200, llama-2-7B's 4096 / 11008, two tables per thread at 512 / 768 / 1024
# threads (4096, 6144, 8192 and the next K), six tables per thread at 512 / 768 / 1024 threads (12288, 18432, 24576, both sides)
KS = [2048, 3200, 4096, 4160, 6144, 6208, 8192, 8256, 11008, 12224, 12288, 12352, 18368, 18432, 18496, 24512, 24576, 24640]
KS_THIN = [2048, 4096, 4160, 11008, 12352, 18496, 24576]
AXES = {
    # row quads: both sides of 1024, 2048, 4096; of the 192..256-workgroup window of twelve-wave workgroups with one (2305..3072), two
    # (1153..1536) and three (769..1024) waves per quad; llama-2-7B: o / down 1024, q/k/v 3072, gate/up 5504 + 2 x 2752 rows = 1376,
    # 3 x 2048 rows = 1536, and the 2- / 4- / 8-way row shards of each
    "tq": [1, 4, 128, 256, 384, 512, 688, 768, 769, 1023, 1024, 1025, 1152, 1153, 1376, 1536, 1537, 2047, 2048, 2049, 2304, 2305, 2752,
           3072, 3073, 4095, 4096, 4097, 5504],
    "tq_thin": [4, 1024, 2049, 4097],
    # rows: both sides of the 256-workgroup rule at one (2040 | 2041) and two (1020 | 1021) waves per quad, and of the grid caps 256 / 512
    "tq_rows": [1, 100, 510, 511, 512, 513, 1020, 1021, 1024, 1025, 2040, 2041, 2048, 2049, 4096, 4097],
    "N": list(range(0, 18)),
    "N_thin": [3, 17],
}
MODES = ["1 0 1", "0 0 1", "1 1 1", "1 0 0", "0 1 0"]      # build_lut dump acc_mfma: need512 off, then on four ways
# every (threads, waves) the kernel has, and some it has not
FORCED = ["%d %d" % c for c in [(512, 1), (512, 2), (768, 1), (768, 2), (768, 3), (1024, 1), (1024, 2), (1024, 4), (768, 4), (640, 0), (512, 4), (1024, 3), (0, 2),
          (768, 0), (0, 3), (1024, 0)]]
AXES["forced"] = FORCED
XF_KINDS = [1, 2, 4, 2 | 1 << 8, 4 | 2 << 8]
# rows: K = 64, then both sides of every step count up to the first K where not even two rows fit (36928), and two K no plan takes.  At every
# K: rows_plan alone ("p") and the launches ("r", at 1024 row quads) over N = 0..17; the row-quad axis is crossed with N = 3 and 17 only
# (N shapes the row groups, the row quads the waves per quad and the grid: neither rule reads the other's input)
KS_ROWS = [64] + [k for n in range(1, 19) for k in (2048 * n, 2048 * n + 64)] + [0, 96]


def cases():
    out = []
    for bits in (1, 2, 3, 4):
        for K in KS:
            for m in MODES:      # the full row-quad axis with need512 off and on; the other ways to need it on the thin one
                out.append(("q %d %d 0 {} %s 0 0" % (bits, K, m), "tq" if m in MODES[:2] else "tq_thin"))
            for strict in (0, 1):
                out.append(("x %d %d 0 {} 1 0 0 %d" % (bits, K, strict), "tq"))
        for K in KS_THIN:
            for tq in AXES["tq_thin"]:
                for m in (MODES[0], MODES[2]):
                    out.append(("q %d %d 0 %d %s {}" % (bits, K, tq, m), "forced"))
                for strict in (0, 1):
                    out.append(("x %d %d 0 %d 1 {} %d" % (bits, K, tq, strict), "forced"))
            for kind in XF_KINDS[1:]:
                out.append(("x %d %d 0 {} %d 0 0 0" % (bits, K, kind), "tq_thin"))
    for bits in (1, 2):      # unified scale: one act group per row
        for K in (4096, 11008, 12352, 24576):
            for m in MODES[:2]:
                out.append(("q %d %d 2 {} %s 0 0" % (bits, K, m), "tq"))
            out.append(("x %d %d 2 {} 4 0 0 0" % (bits, K), "tq"))
    for K in KS_ROWS:
        out.append(("p %d {}" % K, "N"))
        out.append(("r %d {} 1024" % K, "N"))
        for N in AXES["N_thin"] if K <= 24640 else ():      # (beyond: k_gemv_quad's K limit refuses)
            out.append(("r %d %d {}" % (K, N), "tq_rows"))
    return out


def queries(case_list):
    return [t.replace("{}", str(v)) for t, axis in case_list for v in AXES[axis]]


def build_program(tmp):
    exe = os.path.join(tmp, "launch_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "launch_plan_main.cc"),
                    os.path.join(ROOT, "tmac_amd", "csrc", "tmac_launch_plan.cpp")], check=True)
    return exe


def answers(exe, qs):
    """the program's answer lines; the plan without the "| inst" column, and that column (None where the program prints none)"""
    got = subprocess.run([exe], input="\n".join(qs) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(got) == len(qs) and "?" not in got
    plans, inst = [], []
    for line in got:
        plan, sep, flag = line.partition(" | inst ")
        plans.append(plan)
        inst.append(int(flag) if sep else None)
    return plans, inst


def record(exe):
    cl = cases()
    plans, _ = answers(exe, queries(cl))
    distinct = sorted(set(plans))
    index = {p: i for i, p in enumerate(distinct)}
    recorded, at = [], 0
    for t, axis in cl:
        n = len(AXES[axis])
        recorded.append([t, axis, [index[p] for p in plans[at:at + n]]])
        at += n
    body = ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in recorded)
    return '{"axes": %s,\n"answers": %s,\n"cases": [\n%s\n]}\n' % (json.dumps(AXES), json.dumps(distinct, indent=0), body)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe")
    ap.add_argument("--out", default=os.path.join(HERE, "launch_plans.json"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        text = record(args.exe or build_program(tmp))
    with open(args.out, "w") as f:
        f.write(text)
    print("%s: %d bytes, %d queries" % (args.out, len(text), len(queries(cases()))))
