"""What a LUT workspace holds, and which launches put it there, without a GPU: tmac_amd/csrc/tmac_lut_held.h compiled with plain g++ into a
stand-alone program (tests/cpp/lut_held_main.cc: its own main, its own tmac_host::fail).

The planner (lut_build_plan) against an independent restatement of its rules, written here and never read back from the C++, over
K x N x act group size x want x (plain | permutation | transform) x unified x pairs_min_n x image threshold x image buffers; its refusals,
codes, texts and order; the queries of LutHeld after commit and after clear; and the single-writer property of the sources: only
tmac_workspace.cpp calls the LUT builders and moves a workspace's LutHeld.
"""
import glob
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tmac_amd", "csrc")
E_NOMATCH, E_ARG = -1, -4
LB_IMAGE, LB_HALF, LB_ALL = 1, 2, 3                      # enum LutBuild
NONE, PREPROCESS, PAIRS, PAIRS_ROW = 0, 1, 2, 3          # enum LutBuilder
IMG_NONE, IMG_ROWWISE, IMG_CHUNK = 0, 1, 2               # enum LutImage
PAIRS_ROW_MAX_K = 12288
PLAIN, PERM, XF, BOTH = 0, 1, 2, 3
MAXK, MAXN = 12352, 70


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lut_held") / "lut_held_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", path, os.path.join(HERE, "cpp", "lut_held_main.cc")], check=True)
    return path


def parse(line):
    """one output line -> (request tuple, rc, message or None, plan tuple, held tuple, queries tuple)"""
    req, rest = line.rstrip("\n").split("\t|\t", 1)
    req = tuple(int(v) for v in req.split("\t"))
    if rest.count("|") == 0 or not rest.startswith("0\t"):
        rc, msg = rest.split("\t", 1)
        return req, int(rc), msg, None, None, None
    rc, plan, held, qs = rest.split("|\t")
    ints = lambda s: tuple(int(v) for v in s.split())
    return req, int(rc), None, ints(plan), ints(held), ints(qs)


def expected(K, N, ags, want, mode, unified, pairs_min_n, image_min_n, image_buffers):
    """The rules, restated: (rc, fragment of the message) for a refusal, else (0, plan, held).
    plan = (builder, all_layouts, row_image, lut_image); held = (K, N, ags, ref, dev, half, image)"""
    perm, xf = mode == PERM, mode == XF
    # refusals, in their order (the shapes of the sweep pass the shape checks: test_shape_refusals)
    if perm and ags != 64:
        return E_NOMATCH, "the gathered LUT build takes act groups of 64 (act_group_size=%d)" % ags
    if xf and want == LB_ALL:
        return E_NOMATCH, "this plan builds every layout"
    if want == LB_ALL:
        if perm:
            builder = PAIRS                                       # the gather, for every N
        elif ags == 64 and N >= pairs_min_n:
            builder = PAIRS
        elif ags == K and K <= PAIRS_ROW_MAX_K and N >= pairs_min_n:
            builder = PAIRS_ROW
        else:
            builder = PREPROCESS
        wanted = N >= 2 and image_min_n >= 0 and N >= image_min_n and bool(image_buffers)
        lut_image = wanted and ags == 64                          # chunk-major by k_lut_image, whatever the builder; it wins at K == 64
        row_image = wanted and builder == PAIRS_ROW               # row-wise, written by the row-wise pair build itself
        image = IMG_CHUNK if lut_image else IMG_ROWWISE if row_image else IMG_NONE
        return 0, (builder, 1, int(row_image), int(lut_image)), (K, N, ags, 1, 1, 1, image)
    if want == LB_HALF:
        return 0, (PAIRS if ags == 64 else PAIRS_ROW, 0, 0, 0), (K, N, ags, 0, 0, 1, IMG_NONE)
    # LB_IMAGE: no layout is recorded (the workspace serves no LUT query); the image is
    if unified:
        return 0, (PAIRS_ROW, 0, 1, 0), (K, N, ags, 0, 0, 0, IMG_ROWWISE)
    return 0, (NONE, 0, 0, 1), (K, N, ags, 0, 0, 0, IMG_CHUNK)


def test_planner_sweep_and_state(exe):
    out = subprocess.run([exe, "sweep", str(MAXK), str(MAXN)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 5 * 6 * 3 * 3 * 3 * 2 * 2 * 3 * 2
    seen = set()
    for line in out:
        req, rc, msg, plan, held, qs = parse(line)
        K, N, ags, want, mode, unified, pmin, thr, bufs = req
        seen.add((K, N, ags if ags != K else "K", want, mode, pmin, thr, bufs))
        exp = expected(*req)
        if exp[0]:
            assert rc == exp[0] and exp[1] in msg, (req, rc, msg, exp)
            continue
        assert rc == 0, (req, rc, msg)
        assert (plan, held) == exp[1:], (req, plan, held, exp)
        img1, img2, lut1, lutN, lutN1, through, through_other, through_next, exactly, after_clear = qs
        image, layouts = held[6], held[3:6]
        # the image is served iff the plan built one, and only as the kind it built
        assert (img1, img2) == (int(image == IMG_ROWWISE), int(image == IMG_CHUNK)), (req, qs)
        if not (plan[2] or plan[3]):
            assert (img1, img2) == (0, 0), (req, qs)
        # an image implies the LUT of its rows, except behind LB_IMAGE, which serves no LUT query
        assert (lut1, lutN) == ((0, 0) if want == LB_IMAGE else (1, 1)) and lutN1 == 0, (req, qs)
        if (img1 or img2) and want != LB_IMAGE:
            assert lut1 and lutN, (req, qs)
        assert (through, through_other, through_next) == (1, 0, 0), (req, qs)
        assert exactly == layouts[0] == int(want == LB_ALL), (req, qs)
        assert after_clear == 0, req
    assert len(seen) == 5 * 6 * 3 * 3 * 3 * 2 * 3 * 2 - 6 * 3 * 3 * 2 * 3 * 2      # (K = 64: the act group sizes 64 and K are one)


def plan_one(exe, K, N, ags, want=LB_ALL, mode=PLAIN, unified=0, pmin=2, thr=12, bufs=1, maxK=MAXK, maxN=MAXN, perm_K=None):
    args = [K, N, ags, want, mode, unified, pmin, thr, bufs, maxK, maxN, K if perm_K is None else perm_K]
    return parse(subprocess.run([exe, "plan"] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout)


def test_shape_refusals_and_their_order(exe):
    for K, N in ((0, 1), (256, 0), (320, 4), (256, 5)):
        _, rc, msg, *_ = plan_one(exe, K, N, 64, maxK=256, maxN=4)
        assert rc == E_ARG and msg == "K=%d N=%d exceed the workspace (256, 4)" % (K, N)
    for ags in (0, 48, 96, 512):
        _, rc, msg, *_ = plan_one(exe, 256, 2, ags)
        assert rc == E_NOMATCH and msg == "act_group_size=%d must be a multiple of 32 dividing K=256 (qgemm.py:402-404)" % ags
    _, rc, msg, *_ = plan_one(exe, 96, 2, 32)
    assert rc == E_NOMATCH and msg == "K=96 must be a multiple of 64"
    # the workspace's size comes before the act group size, both before the permutation's refusals, the act group size of a gathered
    # build before the permutation's K, and those before the transform's
    _, rc, msg, *_ = plan_one(exe, 512, 2, 48, mode=PERM, maxK=256, perm_K=128)
    assert rc == E_ARG and "exceed the workspace" in msg
    _, rc, msg, *_ = plan_one(exe, 256, 2, 48, mode=PERM, perm_K=128)
    assert rc == E_NOMATCH and "must be a multiple of 32" in msg
    _, rc, msg, *_ = plan_one(exe, 256, 2, 32, mode=PERM, perm_K=128)
    assert rc == E_NOMATCH and msg == "the gathered LUT build takes act groups of 64 (act_group_size=32)"
    _, rc, msg, *_ = plan_one(exe, 256, 2, 64, mode=PERM, perm_K=128)
    assert rc == E_ARG and msg == "the K permutation was built for K=128; the call has K=256"
    _, rc, msg, *_ = plan_one(exe, 256, 2, 64, want=LB_HALF, mode=PERM, perm_K=128)
    assert rc == E_ARG and "was built for K=128" in msg
    # a transform: not with every layout, not together with a permutation; the permutation's own refusals come first
    _, rc, msg, *_ = plan_one(exe, 256, 2, 64, want=LB_ALL, mode=BOTH)
    assert rc == E_NOMATCH and "this plan builds every layout" in msg
    for want in (LB_HALF, LB_IMAGE):
        _, rc, msg, *_ = plan_one(exe, 256, 2, 64, want=want, mode=BOTH)
        assert rc == E_NOMATCH and msg == "a LUT build takes a vector transform or a K permutation, not both"
    _, rc, msg, *_ = plan_one(exe, 256, 2, 64, want=LB_HALF, mode=BOTH, perm_K=128)
    assert rc == E_ARG and "was built for K=128" in msg


def strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_single_writer():
    """Only tmac_workspace.cpp calls the LUT builders; only it clears and commits a LutHeld; nobody assigns one or a member of one
    (tmac_lut_held.h, where the planner fills the plan's, apart)."""
    call = re.compile(r"\b(launch_preprocess\w*|launch_lut_image)\s*\(")
    assign = r"\s*(=(?!=)|\+=|-=|\|=|&=|\+\+|--)"
    member = re.compile(r"(\bheld\b\s*(\.|->)\s*\w+" + assign + r"|(\.|->)\s*held\b" + assign + r"|\b(K_|N_|ags_|layouts_|image_|perm_id_)\b" + assign + ")")
    move = re.compile(r"\bheld\b\s*(\.|->)\s*(clear|commit)\s*\(")
    files = sorted(f for pat in ("*.h", "*.cpp", "*.hip") for f in glob.glob(os.path.join(CSRC, pat)))
    assert len(files) > 30
    callers, movers = set(), set()
    for path in files:
        name = os.path.basename(path)
        with open(path) as f:
            text = strip_comments(f.read())
        for m in call.finditer(text):
            line_start = text.rfind("\n", 0, m.start()) + 1
            if not re.search(r"\bhipError_t\s+$", text[line_start:m.start()]):       # (a declaration or the definition is no call)
                callers.add(name)
        if name == "tmac_lut_held.h":
            continue
        assert not member.search(text), (name, member.search(text).group(0))
        if move.search(text):
            movers.add(name)
    assert callers == {"tmac_workspace.cpp"}, callers
    assert movers == {"tmac_workspace.cpp"}, movers
