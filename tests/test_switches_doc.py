"""docs/SWITCHES.md lists exactly the environment switches the library reads, and the only build-time switches of the
sources are LMN_EMU and LMN_BATCH: an experiment that is left behind as an unlisted getenv or a -D macro fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "luminair_amd", "csrc")


def _sources():
    files = [p for ext in ("*.h", "*.cpp", "*.hip") for p in glob.glob(os.path.join(CSRC, ext))]
    assert len(files) > 30, files
    # a directive continued with a backslash is one line
    return {p: open(p).read().replace("\\\n", " ") for p in files}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_switches_doc_lists_exactly_the_environment_switches_the_library_reads():
    read = set()
    for text in _sources().values():
        read |= set(re.findall(r'\b(?:getenv|env_int|env_set)\(\s*"(LMN_[A-Z0-9_]+)"', _strip_comments(text)))
    listed = set()
    for line in open(os.path.join(ROOT, "docs", "SWITCHES.md")):
        cells = line.split("|")
        if len(cells) >= 4 and cells[0].strip() == "":       # a table row: | variable(s) | default | effect |
            listed |= set(re.findall(r"`(LMN_[A-Z0-9_]+)`", cells[1]))
    assert len(read) >= 20, read                             # the search itself still finds the reads
    assert read == listed, {"read but not listed": sorted(read - listed), "listed but not read": sorted(listed - read)}


def test_the_only_build_time_switches_are_emu_and_batch():
    tested, defined = set(), set()
    for text in _sources().values():
        for line in _strip_comments(text).splitlines():
            m = re.match(r"\s*#\s*(ifdef|ifndef|if|elif)\b(.*)", line)
            if m:
                tested |= set(re.findall(r"\bLMN_[A-Za-z0-9_]+\b", m.group(2)))
            m = re.match(r"\s*#\s*define\s+(LMN_[A-Za-z0-9_]+)", line)
            if m:
                defined.add(m.group(1))
    # (compiler and platform macros - __HIP_DEVICE_COMPILE__, __x86_64__, __SANITIZE_ADDRESS__ ... - carry no LMN_ prefix)
    assert tested - defined == {"LMN_EMU", "LMN_BATCH"}, sorted(tested - defined)
