"""The ctypes signature table (ops/_native.py ``_SIGS``) against the C source: every
``extern "C" int|long dli_*(...)`` definition under csrc/kernels/*.hip has an entry and every
entry equals its definition, letter for letter. A wrong count or type in the table is silent
garbage on the GPU; this needs no GPU and no built library."""
import ctypes
import re
from pathlib import Path

from distributed_llm_inferencing_amd.ops import _native as N

KERNELS = Path(__file__).resolve().parents[1] / "csrc" / "kernels"

_DEF = re.compile(r'extern\s+"C"\s+(int|long)\s+(dli_\w+)\s*\(([^)]*)\)\s*\{')
_LETTER = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_float: "F", ctypes.c_long: "L"}


def _letter(param: str) -> str:
    """One C parameter -> its letter in the table."""
    if "*" in param or re.search(r"\bhipStream_t\b", param):
        return "P"
    words = param.split()[:-1]                     # the type without the parameter's name
    words = [w for w in words if w != "const"]
    if words in (["int"], ["float"], ["long"]):
        return {"int": "I", "float": "F", "long": "L"}[words[0]]
    raise AssertionError(f"parameter type not in the table's alphabet: {param!r}")


def c_signatures(kernels: Path = KERNELS) -> dict:
    """name -> (return type, letters) of every exported dli_* definition."""
    sigs = {}
    for src in sorted(kernels.glob("*.hip")):
        text = re.sub(r"//[^\n]*", "", src.read_text())
        for ret, name, params in _DEF.findall(text):
            assert name not in sigs, f"{name} defined twice"
            params = " ".join(params.split())
            letters = [_letter(p.strip()) for p in params.split(",")] if params else []
            sigs[name] = (ret, "".join(letters))
    return sigs


def test_parser_sees_the_definitions():
    sigs = c_signatures()
    assert len(sigs) >= 40
    # one of each kind: a stream as the last pointer, a long argument, no stream, a long result
    assert sigs["dli_silu_mul"] == ("int", "PPIIP")
    assert sigs["dli_prefetch"] == ("int", "PLIPP")
    assert sigs["dli_decode_set_form"] == ("int", "I")
    assert sigs["dli_decode_attention_workspace_bytes"] == ("long", "IIII")


def test_every_entry_equals_its_definition():
    sigs = c_signatures()
    wrong = {}
    for name, args in N._SIGS.items():
        table = "".join(_LETTER[a] for a in args)
        if name not in sigs:
            wrong[name] = (table, "no definition")
        elif sigs[name][1] != table:
            wrong[name] = (table, sigs[name][1])
    assert not wrong, f"_SIGS entry vs C definition: {wrong}"


def test_every_export_has_an_entry():
    missing = sorted(set(c_signatures()) - set(N._SIGS))
    assert not missing, f"exported but not in _SIGS: {missing}"


def test_long_results_are_the_bytes_functions():
    # _load() gives a c_long restype to the names that end in _bytes and c_int to the rest
    for name, (ret, _) in c_signatures().items():
        assert (ret == "long") == name.endswith("_bytes"), name
