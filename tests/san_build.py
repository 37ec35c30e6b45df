"""A stand-alone C program of the tests, built under ASan and UBSan: its own
main, its own process, nothing of it loaded into this interpreter."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(source, exe):
    """tests/<source> -> exe (a path); the public headers and the library's
    core headers are on the include path.  Asserts a clean compile."""
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                        "-I" + os.path.join(REPO, "include"),
                        "-I" + os.path.join(REPO, "firedancer_amd", "csrc"),
                        os.path.join(REPO, "tests", source), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)
