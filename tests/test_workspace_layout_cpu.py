"""The render workspace's layout (csrc/mdvt_workspace.h) -- no GPU: the header compiled for the host (tests/workspace_layout_host.cpp)
prints what it answers for a sweep of frame sizes, slot counts and bank splits; here every size and offset is compared with a closed
form written out independently (transcribed from the expressions mdvt_api.hip held before the header existed), and the blocks are
checked for what the kernels rely on: nothing outside its allocation, no overlap, the two banks apart, the alignments."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc")

# small, odd, the usual, and the 32-bit queue cap: 4 slots fit at 16384 x 16383, 1 at 32767 x 32767, none at the largest frame
SIZES = [(2, 2), (3, 5), (33, 17), (100, 31), (256, 144), (1920, 1080), (3840, 2160), (16384, 16383), (32767, 32767), (65535, 32767)]
HUGE_CAP, TIE_TILE, REC_DWORDS = 1 << 17, 32, 2


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("layout") / "workspace_layout_host")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                        os.path.join(REPO, "tests", "workspace_layout_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe] + [f"{w}x{h}" for w, h in SIZES], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    fields, out = None, []
    for line in r.stdout.splitlines():
        tag, *rest = line.split()
        if tag == "F":
            fields = rest
        elif tag == "L":
            assert len(rest) == len(fields)
            out.append((dict(zip(fields, map(int, rest))), []))
        else:
            out[-1][1].append(tuple(map(int, rest)))      # (bank_slots, bank 1's counter offset, coarse_at)
    return out


def test_the_sweep_is_complete(cases):
    seen = {(L["W"], L["H"], L["slots"], L["huge_lists"]): [b[0] for b in banks] for L, banks in cases}
    assert set(seen) == {(w, h, s, hl) for w, h in SIZES for s in range(1, 33) for hl in (1, 2)}
    for (_, _, slots, _), bs in seen.items():
        assert bs == list(range(1, slots // 2 + 1))       # every bank_slots with 2 * bank_slots <= slots


def _closed_form(W, H, nf, hl):
    """What mdvt_api.hip computed in ensure_workspace, in the RenderArgs fill of mdvt_render_stereo_batch and in mdvt_debug_read."""
    npx, ntri = W * H, 2 * (W - 1) * (H - 1)
    fit = 0xFFFFFFF0 // (4 * npx)
    cap = min(fit, nf) * npx * 4
    tw = (((W + TIE_TILE - 1) // TIE_TILE) * ((H + TIE_TILE - 1) // TIE_TILE) + 31) // 32
    huge = 2 * HUGE_CAP + 2
    e = dict(W=W, H=H, slots=nf, huge_lists=hl)
    e["plane_bytes"] = nf * npx * 8
    e["tri_invalid_bytes"] = nf * ntri
    e["unused_bytes"] = nf * npx
    e["elist_bytes"] = (nf * 2 * npx + nf * H + nf * npx + nf) * 4
    e["elist_count_at"] = nf * 2 * npx
    e["vlist_at"] = e["elist_count_at"] + nf * H
    e["vlist_count_at"] = e["vlist_at"] + nf * npx
    e["queue_bytes"] = (cap * REC_DWORDS + 2 * nf * H + 8 + hl * huge + nf * (1 + 2 * tw)) * 4
    e["queue_slots"] = min(fit, nf)
    e["bigq_cap"] = cap
    e["counters_at"] = cap * REC_DWORDS
    e["counter_words"] = 2 * nf * H + 8
    e["huge_at"] = e["counters_at"] + 2 * nf * H + 8
    e["huge_list_dwords"] = huge
    e["tie_flag_at"] = e["huge_at"] + hl * huge
    e["tie_tiles_at"] = e["tie_flag_at"] + nf
    e["tie_words"] = tw
    e["elist_stride"] = 2 * W * H                         # a.elist += slot0 * 2 * W * H, and so on
    e["queue_stride"] = H * (4 * W) * REC_DWORDS
    e["tie_tiles_stride"] = 2 * tw
    e["queue_slots_max"] = fit
    e["nominal"] = W * H * (16 + 16 + 32)                 # the budget's contract (include/mdvt.h, workspace_mib)
    e["nominal_edge_flags"] = W * H * (64 + 3)
    e["nominal_edge_points"] = W * H * (64 + 28 + 3)
    return e


def test_every_size_and_offset_equals_its_closed_form(cases):
    for L, banks in cases:
        assert L == _closed_form(L["W"], L["H"], L["slots"], L["huge_lists"])
        for bs, off1, coarse_at in banks:
            assert off1 == (2 * bs * L["H"] + 2 + 3) & ~3
            assert coarse_at == bs * L["H"]


def _tiles(blocks, end):
    """blocks: (name, first, words) in address order -- each inside [0, end), none overlapping the one before it."""
    at = 0
    for name, first, words in blocks:
        assert first >= at and first + words <= end, name
        at = first + words


def test_sub_blocks_lie_inside_their_allocation_and_apart(cases):
    for L, _ in cases:
        nf, H, npx = L["slots"], L["H"], L["W"] * L["H"]
        _tiles([("elist", 0, nf * 2 * npx), ("elist_count", L["elist_count_at"], nf * H), ("vlist", L["vlist_at"], nf * npx),
                ("vlist_count", L["vlist_count_at"], nf)], L["elist_bytes"] // 4)
        lists = [(f"huge list {k}", L["huge_at"] + k * L["huge_list_dwords"], L["huge_list_dwords"]) for k in range(L["huge_lists"])]
        _tiles([("entries", 0, L["bigq_cap"] * REC_DWORDS), ("counters", L["counters_at"], L["counter_words"])] + lists +
               [("tie flags", L["tie_flag_at"], nf), ("tie tiles", L["tie_tiles_at"], nf * L["tie_tiles_stride"])], L["queue_bytes"] // 4)
        assert L["elist_bytes"] % 4 == 0 and L["queue_bytes"] % 4 == 0
        # the slots the queue serves have their entries' room; the whole workspace as one launch set has its counters and coarse sums
        assert L["queue_slots"] * L["queue_stride"] == L["bigq_cap"] * REC_DWORDS
        assert nf * H + (nf * H + 1) <= L["counter_words"]


def test_the_two_banks_are_disjoint(cases):
    for L, banks in cases:
        H, npx, ntri = L["H"], L["W"] * L["H"], 2 * (L["W"] - 1) * (L["H"] - 1)      # npx, ntri: the slot strides of the planes and flags
        for bs, off1, coarse_at in banks:
            coarse_max = bs * H + 1      # a word per block of segments and one more: n H + 1 at shift 0 (k_mesh_queue_reset zeroes k <= ncoarse)
            def halves(name, first, stride, room):
                """slots [0, bs) and [bs, 2 bs) of a per-slot array of `room` elements at `first`"""
                _tiles([(name + " bank 0", first, bs * stride), (name + " bank 1", first + bs * stride, bs * stride)], first + room)
            for name, nbytes in (("plane", L["plane_bytes"] // 8), ("unused", L["unused_bytes"])):
                halves(name, 0, npx, nbytes)
            halves("tri_invalid", 0, ntri, L["tri_invalid_bytes"])
            halves("elist", 0, L["elist_stride"], L["elist_count_at"])
            halves("elist_count", L["elist_count_at"], H, L["slots"] * H)
            halves("vlist", L["vlist_at"], npx, L["slots"] * npx)
            halves("vlist_count", L["vlist_count_at"], 1, L["slots"])
            halves("tie flags", L["tie_flag_at"], 1, L["slots"])
            halves("tie tiles", L["tie_tiles_at"], L["tie_tiles_stride"], L["slots"] * L["tie_tiles_stride"])
            # (a general mesh launch set has at most queue_slots_max slots -- chunk_of, mdvt_api.hip -- so banks of more do not occur)
            if 2 * bs <= L["queue_slots"]:
                halves("entries", 0, L["queue_stride"], L["bigq_cap"] * REC_DWORDS)
            # each bank's segment counters and its worst-case coarse sums, inside the counters' room
            assert coarse_at == bs * H
            _tiles([("counters bank 0", 0, coarse_at + coarse_max), ("counters bank 1", off1, coarse_at + coarse_max)], L["counter_words"])
            # each bank's huge list: the second one inside the block (huge_lists = 2) or an allocation of its own
            if L["huge_lists"] == 2:
                assert L["huge_at"] + 2 * L["huge_list_dwords"] <= L["tie_flag_at"]
            assert L["huge_list_dwords"] >= 2 * HUGE_CAP + 2


def test_alignment_and_index_width(cases):
    for L, banks in cases:
        for k in range(L["huge_lists"]):
            assert (L["huge_at"] + k * L["huge_list_dwords"]) * 4 % 8 == 0           # uint2 entries
        assert L["counters_at"] * 4 % 16 == 0
        for bs, off1, _ in banks:
            assert (L["counters_at"] + off1) * 4 % 16 == 0
        # entry indices are 32-bit, an entry's dword index (kBigRecDwords each) is formed from them in 64 bits
        assert L["bigq_cap"] <= 0xFFFFFFF0 and L["bigq_cap"] == L["queue_slots"] * L["W"] * L["H"] * 4
        assert L["queue_slots"] == min(L["slots"], 0xFFFFFFF0 // (4 * L["W"] * L["H"]))
