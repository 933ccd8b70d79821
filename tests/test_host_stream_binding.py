"""The binding takes a stream wherever include/qmg_hip.h does, and tests/test_gpu_streams.py has a case for every such entry point.

The header is parsed the way tests/test_abi_symbols.py parses it.  A stream-taking prototype is one whose last parameter is `void* stream`,
`void* s` or `void* st`; its Python wrapper (the symbol minus `qmg_`, or the name in WRAPPER) must have a `stream` parameter that defaults
to None, the null stream.  The case table of tests/test_gpu_streams.py is then held to that set: header = CASES + EXEMPT, the two
disjoint, EXEMPT within the five names that may be exempt."""
import importlib
import inspect
import os
import re

qmg = importlib.import_module("quantum-mg_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# wrappers whose name is not the symbol minus `qmg_`
WRAPPER = {
    "qmg_stream_sync": "sync",
    "qmg_stencil_apply_mat16_t": "stencil_apply_mat16",
    "qmg_stencil_apply_epi_t": "stencil_apply_epi",
    "qmg_batch_mr_dots_t": "batch_mr_dots",
    "qmg_batch_mr_update_t": "batch_mr_update",
}
MAY_BE_EXEMPT = {"qmg_stream_sync", "qmg_stream_destroy", "qmg_event_record", "qmg_allreduce_sum_f64", "qmg_poison_scratch"}


def stream_taking_symbols():
    text = open(os.path.join(ROOT, "include", "qmg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(qmg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return sorted(name for name, params in protos if re.fullmatch(r"void\s*\*\s*(stream|s|st)", params.split(",")[-1].strip()))


def test_header_has_its_stream_taking_entry_points():
    names = stream_taking_symbols()
    assert len(names) >= 130 and len(set(names)) == len(names), len(names)
    assert set(names) <= set(qmg.ABI_SYMBOLS)
    assert set(WRAPPER) <= set(names)


def test_every_wrapper_takes_a_stream_that_defaults_to_the_null_stream():
    missing = []
    for sym in stream_taking_symbols():
        fn = getattr(qmg, WRAPPER.get(sym, sym[len("qmg_"):]), None)
        if fn is None:
            missing.append((sym, "no wrapper"))
            continue
        p = inspect.signature(fn).parameters.get("stream")
        if sym == "qmg_stream_destroy":     # the stream is the operand, not the place of the work: it has no default
            assert p is not None and p.default is p.empty
            continue
        if p is None or p.default is not None or p.kind not in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY):
            missing.append((sym, "no stream=None"))
    assert not missing, missing


def test_no_wrapper_hands_the_raw_handle_to_ctypes():
    """Without argtypes ctypes passes a Python int as a C int: a stream handle has to go through c_void_p."""
    text = open(os.path.join(ROOT, "quantum-mg_amd", "__init__.py")).read()
    assert not re.findall(r"lib\(\)\.qmg_\w+\((?:[^()]|\([^()]*\))*[, ]stream\)", text)


def test_case_table_covers_the_header():
    streams = importlib.import_module("test_gpu_streams")
    header, cases, exempt = set(stream_taking_symbols()), set(streams.CASES), set(streams.EXEMPT)
    assert exempt <= MAY_BE_EXEMPT, exempt - MAY_BE_EXEMPT
    assert not (cases & exempt), cases & exempt
    assert cases | exempt == header, (sorted(header - cases - exempt), sorted((cases | exempt) - header))
    assert all(streams.CASES[s] for s in cases) and all(isinstance(r, str) and r for r in streams.EXEMPT.values())
    for sym, label in streams.CONTROLS:
        assert label in dict(streams.CASES[sym])


# ---- the audit of the sources: every launch names the caller's stream, every runtime call that takes a stream gets it
CSRC = os.path.join(ROOT, "quantum-mg_amd", "csrc")
STREAM_ARG = re.compile(r"st|(qmg::)?as_stream\((stream|s|st|q\.stream)\)")
# synchronous runtime calls on the null stream, each followed by a device synchronise or a host read of its own (file -> how many)
NULL_STREAM_CALLS = {
    "qmg_batch.hip": 3,     # get_bws: the workspace's zeros, once per thread, a device synchronise behind them
    "qmg_common.h": 1,      # poison_new_scratch: a device synchronise behind it
    "qmg_comm.hip": 2,      # qmg_comm_all_ok: a flag up and its sum down, both synchronous
    "qmg_runtime.hip": 1,   # qmg_memcpy_* with stream == NULL: synchronous by contract
}


def _split_top_level(args):
    parts, cur, depth = [], "", 0
    for ch in args:
        depth += ch in "(["
        depth -= ch in ")]"
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return parts + [cur.strip()]


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            yield name, open(os.path.join(CSRC, name)).read()


def test_every_kernel_launch_names_the_stream_of_its_caller():
    launches, bad = 0, []
    for name, text in _sources():
        for m in re.finditer(r"<<<(.*?)>>>", text, flags=re.S):
            launches += 1
            config = _split_top_level(m.group(1))
            if len(config) != 4 or not STREAM_ARG.fullmatch(config[3]):
                bad.append((name, text[:m.start()].count("\n") + 1, config[-1]))
    assert launches >= 180, launches     # the scan still finds the launch sites (185 today)
    assert not bad, bad


def test_runtime_copies_and_memsets_take_the_stream():
    found = {}
    for name, text in _sources():
        text = re.sub(r"//[^\n]*", "", text)
        n = len(re.findall(r"\bhipMem(?:cpy|set|cpy2D)\s*\(", text))
        if n:
            found[name] = n
        for m in re.finditer(r"\bhipMem(?:cpy|set)Async\s*\(((?:[^()]|\((?:[^()]|\([^()]*\))*\))*)\)", text):
            last = _split_top_level(m.group(1))[-1]
            assert re.fullmatch(r"st|as_stream\((stream|st|s)\)|\(hipStream_t\)\s*stream", last), (name, m.group(0)[:120])
    assert found == NULL_STREAM_CALLS, found


def test_the_workspace_zeros_are_synchronised_before_their_first_use():
    """get_bws zeroes `done`, `result` and `mr` on the null stream; the thread's first reduction may run on a non-blocking stream."""
    text = open(os.path.join(CSRC, "qmg_batch.hip")).read()
    body = text[text.index("int get_bws("):text.index("void release_batch_workspace")]
    last_memset = body.rindex("hipMemset(")
    assert "hipDeviceSynchronize()" in body[last_memset:body.index("g_bws.device = dev")]
