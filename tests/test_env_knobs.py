"""Every PGA_* environment variable the code reads is documented.

The names are collected from the getenv( / os.environ calls under csrc/,
libpga_amd/ and tools/build.py; each must appear in README's `Environment:`
paragraph or in docs/ARCHITECTURE.md, so the knob list cannot grow unseen.
"""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
READ = re.compile(r"(?:getenv\(|os\.environ\b[^\n]*?)\s*[\[(]?\s*\"(PGA_[A-Z0-9_]+)\"")


def sources():
    for top in ("csrc", "libpga_amd"):
        for p in sorted((ROOT / top).rglob("*")):
            if p.is_file() and p.suffix in (".cpp", ".hpp", ".hip", ".h", ".c", ".py"):
                yield p
    yield ROOT / "tools" / "build.py"


def knobs_read():
    found = {}
    for p in sources():
        for name in READ.findall(p.read_text(errors="replace")):
            found.setdefault(name, p.relative_to(ROOT).as_posix())
    return found


def environment_paragraph():
    text = (ROOT / "README.md").read_text()
    start = text.index("Environment:")
    end = text.find("\n\n", start)
    return text[start:end if end >= 0 else len(text)]


def test_every_env_knob_is_documented():
    found = knobs_read()
    # the scan itself works: these three are read by the engine, the package and the build
    assert {"PGA_TP_SKEW", "PGA_LOG", "PGA_ARCH"} <= set(found)
    documented = environment_paragraph() + (ROOT / "docs" / "ARCHITECTURE.md").read_text()
    missing = {n: f for n, f in found.items() if not re.search(rf"\b{n}\b", documented)}
    assert not missing, f"undocumented environment variables (name: first file that reads it): {missing}"
