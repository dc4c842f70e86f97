"""csrc/dispatch.h on the host: every selector value reaches its own tag exactly once, a value outside a one_of list is an error
(BBDM_E_BADARG + a message) and calls nothing.  Compiled against the emulator's HIP header, as tools/hipemu compiles the launchers."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "hipemu"))

PROGRAM = r"""
#include <initializer_list>
#include <stdarg.h>
#include <string.h>
#include "dispatch.h"
static char g_err[256];
static int g_set = 0;
void bbdm_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); ++g_set; }
template <int M, bool A, bool B> int leaf() { return M * 100 + A * 10 + B; }
int main() {
    int calls = 0;
    auto f = [&](auto M, auto A, auto B) { ++calls; return leaf<M(), A(), B()>(); };
    for (int m : {2, 4, 8, 6})
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                const int before = calls;
                if (dispatch(f, one_of<2, 4, 8, 6>(m), a != 0, b != 0) != m * 100 + a * 10 + b || calls != before + 1) return 1;
            }
    if (dispatch([] { return 7; }) != 7) return 2;
    if (g_set != 0) return 3;
    const int before = calls;
    if (dispatch(f, one_of<2, 4, 8, 6>(5), true, false) != BBDM_E_BADARG || calls != before) return 4;
    if (g_set != 1 || !strstr(g_err, "5")) return 5;
    // a selector after a bool, and a list of one
    if (dispatch([](auto A, auto M) { return A() ? M() : -M(); }, false, one_of<3>(3)) != -3) return 6;
    printf("ok %d\n", calls);
    return 0;
}
"""


def test_dispatch_routes_every_value_once_and_rejects_the_rest(tmp_path):
    import build as hipemu_build
    src = tmp_path / "dispatch_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "dispatch_check"
    subprocess.check_call([hipemu_build.CLANG, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-attributes",
                           "-I", hipemu_build.HERE, "-I", hipemu_build.CSRC, str(src), os.path.join(hipemu_build.HERE, "hipemu.cpp"),
                           "-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.strip() == "ok 16"
