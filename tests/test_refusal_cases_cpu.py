"""tests/refusal_cases.py held to the headers and to csrc/mdvt_api.hip, without a GPU: every entry point the unit defines has a
table entry whose arguments are the declaration's, in its order and of a fitting kind; every pointer, pitch, stride, count, size
and flag parameter is given a wrong value by some case or is exempt for one of the two admissible reasons; the regions the
pointers go to are apart; and the golden file has exactly the table's cases."""
import glob
import os
import re

import footprint as fp
import refusal_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API_UNIT = os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc", "mdvt_api.hip")


def _declarations():
    """{name: [(type text, parameter name)]} of every entry point the headers of include/ declare."""
    out = {}
    for path in sorted(glob.glob(os.path.join(REPO, "include", "*.h"))):
        decl = dict(fp.header_entry_points(path))
        text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
        for m in re.finditer(r"\bconst\s+char\s*\*\s*(mdvt_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):      # the *_supported calls
            decl[m.group(1)] = " ".join(m.group(2).split())
        for name, args in decl.items():
            params = []
            for a in args.split(","):
                a = re.sub(r"\[\d*\]", "*", a.strip())
                m = re.match(r"(.*?)(\w+)$", a)
                if m and a != "void":
                    params.append((m.group(1).strip(), m.group(2)))
            out[name] = params
    return out


def _defined_in_api_unit():
    return re.findall(r"^(?:int|const char\*) (mdvt_\w+)\(", open(API_UNIT).read(), flags=re.M)


def _wanted_kinds(ctype, name):
    """The kinds of refusal_cases.py a parameter of this declaration may have."""
    if ctype.startswith("mdvt_ctx"):
        return ("ctx",)
    if name == "stream":
        return ("stream",)
    if "*" in ctype:
        return ("ptr", "host")
    if ctype == "double":
        return ("depth", "val")
    if re.search(r"(^|_)pitch$", name):
        return ("pitch",)
    if re.search(r"(^|_)stride$", name):
        return ("stride",)
    if ctype in ("size_t", "uint64_t"):
        return ("size", "val")
    assert ctype == "int", (ctype, name)
    return ("count", "flag", "val")


def test_every_entry_point_of_the_api_unit_has_a_table_entry():
    defined = _defined_in_api_unit()
    assert len(defined) >= 31 and len(set(defined)) == len(defined)
    assert sorted(defined) == sorted(e.name for e in rc.TABLE if e.name not in rc.RENDER_UNIT)
    assert [e.name for e in rc.TABLE[-len(rc.RENDER_UNIT):]] == list(rc.RENDER_UNIT)      # (mdvt_api_render.hip's two come last)
    ctxless = [e.name for e in rc.TABLE if "ctx" not in e.by_name]
    assert sorted(ctxless) == ["mdvt_equirect_tables", "mdvt_ffv1_decode_supported", "mdvt_ffv1_packet_is_key", "mdvt_ffv1_stream_decode_supported"]


def test_the_table_follows_the_declarations():
    decl = _declarations()
    for e in rc.TABLE:
        params = decl[e.name]
        assert [p[1] for p in params] == [a.name for a in e.args], e.name
        for (ctype, name), a in zip(params, e.args):
            assert a.kind in _wanted_kinds(ctype, name), f"{e.name}: {ctype} {name} is listed as {a.kind}"


def test_every_parameter_is_mutated_or_exempt():
    decl = _declarations()
    reasons = (rc.NO_VALUE_REFUSED, "the refusal needs an allocation failure or a HIP error")
    for key, why in rc.EXEMPT.items():
        assert why.startswith(reasons), f"{key}: not an admissible reason: {why}"
        assert key[0] in rc.BY_NAME and key[1] in rc.BY_NAME[key[0]].by_name, key
    for e in rc.TABLE:
        mutated = e.mutated()
        for ctype, name in decl[e.name]:
            if ctype.startswith("mdvt_ctx") or ctype == "double":        # (a NULL ctx has no text to pin; doubles: depth-like ones are listed)
                continue
            assert (name in mutated) != ((e.name, name) in rc.EXEMPT), f"{e.name}: {name} must be given a wrong value by a case or be exempt (not both)"
        # the doubles the unit holds to "> 0" are tried at 0.0, NaN and -1.0
        for a in e.args:
            if a.kind == "depth":
                assert sum(1 for label, _ in e.cases() if label.startswith(a.name + " ")) == 3


def test_sizes_and_regions():
    at, total = rc.layout()
    spans = sorted((off, off + rc.BY_NAME[e].by_name[a].value) for (e, a), off in at.items())
    assert spans[0][0] >= rc.MARGIN and total < 1 << 20
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert start - end >= 2 * rc.MARGIN
    for e in rc.TABLE:
        for a in e.args:
            if a.kind == "count" and re.search(r"(width|height|_w|_h)$", a.name) and not a.name.startswith("slices"):
                assert 4 <= a.value <= 16, (e.name, a.name)
        for label, wrong in e.extra:                     # a misaligned pointer stays inside its own margin
            assert all(v.by < rc.MARGIN for v in wrong.values() if isinstance(v, rc.Misaligned))


def test_the_golden_file_has_the_tables_cases():
    golden = rc.load_golden()
    assert list(golden) == [e.name for e in rc.TABLE]
    n = 0
    for e in rc.TABLE:
        assert list(golden[e.name]) == [label for label, _ in e.all_cases()], e.name
        n += len(golden[e.name])
        for a in e.args:                                 # every refusal the mutations were written for is in the file
            if a.kind in ("pitch", "count") and a.name not in ("max_rounds", "first_out", "n_mask_frames"):
                assert any(golden[e.name][label][0] != 0 for label, w in e.cases() if a.name in w), (e.name, a.name)
    assert n >= 900
