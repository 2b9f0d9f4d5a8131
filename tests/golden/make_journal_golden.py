"""Writes tests/golden/journal_ref_lines.npz: the line oracle/_ref/ref_long_trace (the UNMODIFIED reference Predictor behind oracle/ref_harness.cpp)
prints for the `stream` and `vocab` of the trace fixtures text_96 and binary_64 -- the block's end byte position, 130 column-group digests and the
digest of the final probability. Both streams are shorter than a 64 KB block, so each gives one line. tests/test_journal_model.py pins the numpy
model (cmix_amd/journal.py) on these lines, the GPU tests then compare the journal kernel with the model on the same fixtures' rows.

    make -C oracle _ref/libcmixref.so _ref/ref_long_trace && python tests/golden/make_journal_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TOOL = os.path.join(ROOT, "oracle", "_ref", "ref_long_trace")
FIXTURES = ("text_96", "binary_64")


def ref_line(stream, vocab):
    with tempfile.TemporaryDirectory() as d:
        np.asarray(stream, np.uint8).tofile(os.path.join(d, "stream.bin"))
        np.asarray(vocab, np.uint8).tofile(os.path.join(d, "vocab.bin"))
        env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(TOOL) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
        subprocess.check_call([TOOL, os.path.join(d, "stream.bin"), os.path.join(d, "vocab.bin"), os.path.join(d, "out.txt")], env=env)
        lines = [l.split() for l in open(os.path.join(d, "out.txt")) if l.strip()]
    assert len(lines) == 1 and len(lines[0]) == 132, "one block of 131 digests expected"
    return int(lines[0][0]), np.array([int(x, 16) for x in lines[0][1:]], np.uint64)


def main():
    if not os.path.exists(TOOL):
        sys.exit("%s is not built (make -C oracle _ref/libcmixref.so _ref/ref_long_trace)" % TOOL)
    out = {}
    for name in FIXTURES:
        with np.load(os.path.join(HERE, name + ".npz")) as z:
            end, words = ref_line(z["stream"], z["vocab"])
        out[name + "_end"] = np.uint64(end)
        out[name + "_words"] = words
        print(name, end, "%016x ... %016x" % (int(words[0]), int(words[130])))
    np.savez(os.path.join(HERE, "journal_ref_lines.npz"), **out)


if __name__ == "__main__":
    main()
