"""
The host path of the one-tree search and commit calls (refine, connect, via, reach), from the source text: the order that makes a
call safe is written in the two solo runners of csrc/engine_refine.hpp and nowhere else in the calls' fragments, every call
goes through them, and one scratch serves them all.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lqrrt_amd", "csrc")


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def _runners():
    refine = _text("engine_refine.hpp")
    search = refine[refine.index("static int solo_search_run("):refine.index("static int solo_commit_run(")]
    commit = refine[refine.index("static int solo_commit_run("):refine.index("static void refine_decode(")]
    return refine, search, commit


def _solo_halves():
    """The one-tree part of the four fragments (engine_refine.hpp and engine_connect.hpp go on with the calls for several trees)."""
    refine, connect = _text("engine_refine.hpp"), _text("engine_connect.hpp")
    return {"engine_refine.hpp": refine[:refine.index("// Several engines per call")],
            "engine_connect.hpp": connect[:connect.index("// Several trees per call")],
            "engine_connect_via.hpp": _text("engine_connect_via.hpp"),
            "engine_reach.hpp": _text("engine_reach.hpp")}


def test_the_safe_order_stands_in_the_two_runners_only():
    refine, search, commit = _runners()
    guard = refine[refine.index("struct StreamDrain {"):]
    guard = guard[:guard.index("\n};\n")]
    for f, text in _solo_halves().items():
        rest = text.replace(search, "").replace(commit, "").replace(guard, "")
        for word in ("StreamDrain drain(", "drain.arm();", "drain.disarm();", "hipStreamSynchronize(", "hipMemcpyAsync(", "hipGetLastError(",
                     "use_device(e)", "DISPATCH(", "dalloc(", "hipMalloc"):
            assert word not in rest, (f, word)
    for run in (search, commit):
        for word in ("use_device(e)", "solo_scratch(", "StreamDrain drain(st);", "drain.arm();", "hipStreamSynchronize(", "drain.disarm();",
                     "DISPATCH(e, h.template launch<S>(", "hipGetLastError()", "hipMemcpyHostToDevice", "hipMemcpyAsync("):
            assert run.count(word) == (2 if word == "hipMemcpyAsync(" else 1), word    # one copy up, one back
        order = [run.index(w) for w in ("use_device(e)", "solo_scratch(", "std::vector<char> img(", "StreamDrain drain(st);", "h.fill(", "drain.arm();",
                                        "hipMemcpyAsync(", "DISPATCH(", "hipGetLastError()", "hipMemcpyDeviceToHost", "hipStreamSynchronize(st)",
                                        "drain.disarm();")]
        assert order == sorted(order), order
        assert "e->d_solo" in run and "refine_lds_bytes(e, horizon)" in run
    # a search reads back its keys only, into the head of the image the guard stands behind; no launch, no device
    assert "unsigned long long* key = (unsigned long long*)img.data();" in search and "hipMemcpyAsync(key, e->d_solo, " in search
    assert search.index("if (groups == 0) return 0;") < search.index("use_device(e)")
    assert "sizeof(unsigned long long) * keys, hipMemcpyDeviceToHost" in search and "h.won((int)t, key[t])" in search
    # a commit runs on one workgroup's launch (the hooks say dim3(1)), reads out[3], refuses, then adopts
    assert commit.index("int out[3]") < commit.index("StreamDrain drain(st);")
    order = [commit.index(w) for w in ("drain.disarm();", "LQRRT_E_CAPACITY", "LQRRT_E_STATE", "e->tv.elen + base", "refine_adopt(")]
    assert order == sorted(order), order


def test_every_solo_call_goes_through_a_runner():
    halves = _solo_halves()
    calls = {"engine_refine.hpp": (("lqrrt_refine_search", "solo_search_run", "RefineSearchSolo{"), ("lqrrt_refine_commit", "solo_commit_run", "RefineCommitSolo{")),
             "engine_connect.hpp": (("lqrrt_connect_search", "solo_search_run", "ConnectSearchSolo h{"), ("connect_commit_run", "solo_commit_run", "RefineCommitSolo{")),
             "engine_connect_via.hpp": (("lqrrt_connect_via_search", "solo_search_run", "ConnectViaSearchSolo h{"),
                                        ("lqrrt_connect_via_commit", "solo_commit_run", "ConnectViaCommitSolo{")),
             "engine_reach.hpp": (("lqrrt_reach_search", "solo_search_run", "ReachSearchSolo h{"),)}
    for f, rows in calls.items():
        for name, runner, hooks in rows:
            text = halves[f]
            body = text[text.index(" int %s(" % name):]
            body = body[:body.index("\n}\n")]
            # the runner is the call's last statement, behind every refusal of its own
            assert body.count("return %s(" % runner) == 1 and hooks in body, name
            assert "fail(" not in body[body.index("return %s(" % runner):].replace("strf(", ""), name
    assert "return connect_commit_run(" in halves["engine_connect.hpp"] and "return connect_commit_run(" in halves["engine_reach.hpp"]
    # each hooks object names its kernel in its one launch; the replays run on one workgroup
    kernels = {"RefineSearchSolo": "k_refine_search<S>", "RefineCommitSolo": "k_refine_commit<S>", "ConnectSearchSolo": "k_connect_search<S>",
               "ConnectViaSearchSolo": "k_connect_via_search<S>", "ConnectViaCommitSolo": "k_connect_via_commit<S>", "ReachSearchSolo": "k_reach_search<S>"}
    text = "".join(halves.values())
    for hooks, kernel in kernels.items():
        body = text[text.index("struct %s " % hooks):]
        body = body[:body.index("\n};\n")]
        assert body.count("hipLaunchKernelGGL(") == 1 and "hipLaunchKernelGGL((%s)" % kernel in body, hooks
        assert ("dim3(1), dim3(64)" in body) == ("Commit" in hooks), hooks
    assert text.count("hipLaunchKernelGGL(") == len(kernels)


def test_one_scratch_and_one_commit_finish():
    texts = {f: _text(f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".def"))}
    for f, text in texts.items():
        for gone in (r"\bd_ref\b", r"\bref_cap\b", r"\bd_ref_key\b", r"\bd_con\b", r"\bcon_cap\b", r"\bconnect_scratch\b", r"\brefine_prepare\b"):
            assert not re.search(gone, text), (f, gone)
    assert sum(t.count("static int commit_finish(") for t in texts.values()) == 1 and "static int commit_finish(" in texts["engine_wave.hpp"]
    assert sum(t.count("static int solo_scratch(") for t in texts.values()) == 1
    refine = texts["engine_refine.hpp"]
    assert "static int solo_scratch(lqrrt_engine* e, size_t bytes) { return scratch_grow(&e->d_solo, &e->solo_cap, bytes); }" in refine
    grow = refine[refine.index("static int scratch_grow("):]
    grow = grow[:grow.index("\n}\n")]
    assert "dalloc_transient(mem, want)" in grow and "dalloc(" not in grow and "/ 4096 * 4096" in grow   # on demand, outside the footprint
    assert sum(t.count("solo_scratch(") for t in texts.values()) == 3                     # its definition and the two runners
    assert "e->d_solo" in texts["engine_lifecycle.hpp"] and "char* d_solo = nullptr;" in texts["engine_state.hpp"]
    # no fragment but the runners' touches the scratch
    for f, text in texts.items():
        if f not in ("engine_refine.hpp", "engine_lifecycle.hpp", "engine_state.hpp"):
            assert "d_solo" not in text, f
