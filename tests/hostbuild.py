"""The one compile recipe of the tests' host builds.

* shim(name, source_text): shipped headers behind a few extern "C" lines, as a shared library for ctypes.  No sanitizer.
* program(source_file): a program of its own under tests/c, built with -fsanitize=address,undefined and run as a child
  process.

Both are built -ffp-contract=off -fno-fast-math as the library is, with include/, vorbis_amd/csrc and tests/emul on the
include path.  A caller passes only the flags that are its own.  What was built is remembered for the life of the process
(by name, source text and flags) in one temporary directory made at first use."""
import atexit
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ["-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas"]
INCLUDES = ["-I" + os.path.join(ROOT, *p) for p in (("include",), ("vorbis_amd", "csrc"), ("tests", "emul"))]
SHIM = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + CONTRACT + INCLUDES
PROGRAM = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + CONTRACT + INCLUDES

_built = {}
_dir = []


def _build(key, recipe, extra, source, out):
    if key not in _built:
        if not _dir:
            _dir.append(tempfile.mkdtemp(prefix="vamd_hostbuild"))
            atexit.register(shutil.rmtree, _dir[0], ignore_errors=True)
        sub = os.path.join(_dir[0], str(len(_built)))
        os.mkdir(sub)
        src, target = source(sub), os.path.join(sub, out)
        subprocess.check_call(recipe + list(extra) + [src, "-o", target])
        _built[key] = target
    return _built[key]


def shim(name, source_text, extra=()):
    """-> the path of the shared library of `source_text`"""
    def source(sub):
        path = os.path.join(sub, name + "_shim.cpp")
        with open(path, "w") as f:
            f.write(source_text)
        return path
    return _build((name, source_text, tuple(extra)), SHIM, extra, source, "lib%s_host.so" % name)


def program(source_file, extra=()):
    """-> the path of the sanitized executable of tests/c/<source_file>"""
    path = os.path.join(ROOT, "tests", "c", source_file)
    with open(path) as f:
        text = f.read()
    return _build((source_file, text, tuple(extra)), PROGRAM, extra, lambda sub: path, os.path.splitext(source_file)[0])


def run_ok(exe, args=()):
    """Runs a case program: exit status 0 and an output that ends with ": ok".  -> its output"""
    r = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith(": ok"), r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout
