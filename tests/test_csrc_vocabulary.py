"""The lane vocabulary of csrc/  is written once: the sources are read as text, no GPU.

* the bf16 round trip ``bf16_to_f32(f32_to_bf16(`` stands in csrc/lane_math.h alone (as_stored / as_stored4);
* ``keep_if(float4`` and ``mfma16(`` have one definition each, in that header.
"""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nas-segm-pytorch_amd", "csrc")
SHARED = "lane_math.h"

# Sites deliberately left open-coded, as {file: reason}.  Empty: every copy of the three pieces below went into the
# shared header with the kernels' assembly unchanged.  (The sites that keep OTHER algebra written out - the mask with a
# run-time int activation, a few xhat and coefficient blocks - are listed in DESIGN 3.1.1; nothing here looks for them.)
ALLOW_ROUNDING = {}


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) > 20, files
    return {os.path.basename(f): open(f).read() for f in files}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_storage_rounding_is_written_once():
    holders = [name for name, text in _sources().items()
               if "bf16_to_f32(f32_to_bf16(" in _strip_comments(text) and name not in ALLOW_ROUNDING]
    assert holders == [SHARED], holders
    # ... and there once per helper: the scalar form and the four components of the float4 form
    assert _strip_comments(_sources()[SHARED]).count("bf16_to_f32(f32_to_bf16(") == 5


def _definitions(pattern):
    """(file, line) of every function DEFINITION matching `pattern` (a call has no return type in front)"""
    found = []
    for name, text in _sources().items():
        for m in re.finditer(pattern, _strip_comments(text)):
            found.append((name, m.group(0)))
    return found


def test_keep_if_and_mfma16_are_defined_once():
    keep4 = _definitions(r"\bfloat4\s+keep_if\s*\(\s*float4\b")
    assert [f for f, _ in keep4] == [SHARED], keep4
    keep1 = _definitions(r"\bfloat\s+keep_if\s*\(\s*float\b")
    assert [f for f, _ in keep1] == [SHARED], keep1
    mfma = _definitions(r"\bf32x4\s+mfma16\s*\(")
    assert [f for f, _ in mfma] == [SHARED], mfma
    # the private copies and wrappers are gone
    for name, text in _sources().items():
        code = _strip_comments(text)
        for gone in ("keep_if4(", "keep4(", "round_like_storage("):
            assert gone not in code, (name, gone)


def test_every_source_sees_the_shared_header():
    assert re.search(r'^#include "lane_math.h"', _sources()["common.h"], flags=re.M)
