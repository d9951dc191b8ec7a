"""fm3d_pipeline_describe's host side, no GPU: the header declares the call, its two source constants
and fm3d_describe_stats; the Python mirror has the C compiler's size and offsets; the library exports
the symbol.  (tests/test_cmake.py builds the tree with csrc/fm3d_tail.cpp in it.)"""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "fm3d.h")) as f:
        return f.read()


def test_header_declares_the_call():
    text = header()
    assert re.search(r"#define\s+FM3D_DESCRIBE_RECORDS\s+0\b", text)
    assert re.search(r"#define\s+FM3D_DESCRIBE_NCC\s+1\b", text)
    assert re.search(r"typedef struct fm3d_describe_stats\s*\{[^}]*\}\s*fm3d_describe_stats;", text)
    decl = re.search(r"int fm3d_pipeline_describe\(([^;]*)\);", text)
    assert decl, "fm3d_pipeline_describe is not declared"
    args = " ".join(decl.group(1).split())
    assert args == ("fm3d_ctx *ctx, int source, const fm3d_record *recordsDev, int n, void *desc, double *frames, "
                    "uint8_t *patches, fm3d_describe_stats *stats")


def test_stats_mirror_has_the_c_layout(fm3d, tmp_path):
    fields = [f for f, _ in fm3d.DescribeStats._fields_]
    assert fields == ["points", "patchSize", "cols", "type", "chunks", "total_ms"]
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"fm3d.h\"\n"
           "int main(void){printf(\"%zu\\n\", sizeof(fm3d_describe_stats));"
           + "".join(f'printf("%zu\\n", offsetof(fm3d_describe_stats, {f}));' for f in fields)
           + "printf(\"%d %d\\n\", FM3D_DESCRIBE_RECORDS, FM3D_DESCRIBE_NCC);return 0;}")
    c, exe = tmp_path / "s.c", tmp_path / "s"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(fm3d.DescribeStats) == 32
    assert [int(v) for v in out[1:1 + len(fields)]] == [getattr(fm3d.DescribeStats, f).offset for f in fields]
    assert [int(v) for v in out[1 + len(fields):]] == [fm3d.DESCRIBE_SOURCES["records"], fm3d.DESCRIBE_SOURCES["ncc"]]


def test_library_exports_the_symbol(fm3d):
    assert "fm3d_pipeline_describe" in fm3d.EXPORTS
    assert hasattr(fm3d.lib(), "fm3d_pipeline_describe")
    assert hasattr(fm3d.Pipeline, "describe")


def test_both_builds_list_the_new_translation_unit():
    with open(os.path.join(ROOT, "3dfeaturematcher_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS\s*=.*\bfm3d_tail\.cpp\b", f.read(), re.M)
    with open(os.path.join(ROOT, "CMakeLists.txt")) as f:
        assert "${FM3D_CSRC}/fm3d_tail.cpp" in f.read()
