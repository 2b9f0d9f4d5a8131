"""CPU: what the paq8 stage's HOST front end (cmix_amd/csrc/p8front/) shares with the oracle, and what it does not.
  * The parsers with no learner of their own -- p8f_{stem,text,word,xml,record,exe}.c, p8f_stem.h and the four generated table headers (paq8's and fxcm's) -- exist
    ONCE, in the product's tree. The oracle's Makefile compiles the same files a second time with their p8f_* names mapped onto its CPU learners
    (oracle/paq8_names.h), so the class-level tests against the unmodified reference (tests/test_oracle_paq8core.py) pin the
    text that ships. Guarded here: no second copy comes back, and both builds see <ctype.h> as the "C" locale's (the reference never calls setlocale(); a
    difference there sits in a force-included header, where no comparison of the sources would see it).
  * p8f_{match,lpm,ctxmodels}.c differ from oracle/paq8_{match,lpm,ctxmodels}.c in substance (the product emits records for maps that learn on the device, the
    oracle predicts in place) and stay prefix-renamed twins: comment- and prefix-normalised, the line difference of each pair may not grow past what it is today.
    A comparison of one twin with the other proves nothing about either; what pins them is the reference, through the host emulation's per-step hashes
    (tests/test_p8stage_host.py) and on the device.
  * the PRODUCT objects themselves are pinned where they can run alone: the stemmer tests of tests/test_oracle_paq8core.py run again with libcmixamd.so's p8f_*
    entry points in the oracle's place."""
import difflib
import os
import re
import subprocess

import pytest

from conftest import ROOT
from oracle import oracle as O
from oracle import refharness as R

# pair -> the normalised line difference on the day this test was written (round 5); a change to one file that is not mirrored in the other raises it
PAIRS = {"match": 9, "ctxmodels": 30, "lpm": 15}
# the files the oracle builds from the product's tree: one copy each
SHARED = ["p8f_%s.c" % n for n in ("stem", "text", "word", "xml", "record", "exe")] + [
    "p8f_stem.h", "p8f_tables.h", "p8f_stem_tables.h", "cmx_fxcm_tables.h", "cmx_fxcm_stem_tables.h"]


def _norm(path, product):
    s = open(path).read()
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    s = re.sub(r"//[^\n]*", "", s)
    for a in (("p8f_", "P8F_") if product else ("orc_p8_", "ORC_P8_", "orc_", "ORC_")):
        s = s.replace(a, "X_")
    return [x for x in (re.sub(r"\s+", " ", l).strip() for l in s.split("\n")) if x]


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_front_end_and_oracle_twin_have_not_drifted(name):
    a = _norm(os.path.join(ROOT, "cmix_amd", "csrc", "p8front", "p8f_%s.c" % name), True)
    b = _norm(os.path.join(ROOT, "oracle", "paq8_%s.c" % name), False)
    same = sum(m.size for m in difflib.SequenceMatcher(None, a, b, autojunk=False).get_matching_blocks())
    diff = max(len(a), len(b)) - same
    assert diff <= PAIRS[name], "p8f_%s.c and oracle/paq8_%s.c differ in %d normalised lines (%d when the guard was written): mirror the change in the twin" % (name, name, diff, PAIRS[name])


def test_shared_parser_files_exist_once():
    """every shared file is where the product has it, and no file name under cmix_amd/csrc/ comes back under oracle/: neither under the product's name nor
    under the name its copy had there (paq8_* / fxcm_*). A copy would drift again."""
    product = {f for _, _, files in os.walk(os.path.join(ROOT, "cmix_amd", "csrc")) for f in files}
    oracle = set(os.listdir(os.path.join(ROOT, "oracle")))
    assert not [f for f in SHARED if f not in product]
    assert not sorted(product & oracle)
    assert not sorted({f.replace("p8f_", "paq8_").replace("cmx_fxcm_", "fxcm_") for f in SHARED} & oracle)


def test_oracle_library_uses_no_locale_dependent_ctype():
    """libc's tolower / isalpha / ... follow LC_CTYPE (Python calls setlocale at start-up, the reference never does) and show as __ctype_*_loc imports"""
    out = subprocess.check_output(["nm", "-D", "--undefined-only", O.build()], text=True)
    assert not [l for l in out.splitlines() if "__ctype_" in l]


class _ProductAsOracle:
    """the product library answering to the oracle's names: orc_p8_x -> p8f_x (same signatures: one source builds both)"""

    def __init__(self, product, oracle):
        self._p, self._o = product, oracle

    def __getattr__(self, name):
        if name.startswith("orc_p8_") and hasattr(self._p, "p8f_" + name[7:]):
            return getattr(self._p, "p8f_" + name[7:])
        return getattr(self._o, name)


needs_ref = pytest.mark.skipif(not R.paq8core_available(), reason="oracle/_ref/libcmixrefpaq8.so not built")


@needs_ref
@pytest.mark.parametrize("case", ["test_english_stemmer_vs_reference", "test_french_and_german_stemmers_vs_reference"])
def test_product_front_end_objects_vs_reference(case, monkeypatch):
    """The stemmers are the self-contained part of the front end (stem letters, flags, both hash sets of every word against the reference's EnglishStemmer /
    FrenchStemmer / GermanStemmer). The sub-models (word, text, XML, record, exe, match, linear prediction) hand their contexts to the emitter of the chunk
    being built instead of to ContextMaps of their own, so they cannot run stand-alone; they are pinned one level up, by the per-step hashes of the unmodified
    paq8::Predictor through the stage's host emulation (tests/test_p8stage_host.py::test_stage_vs_reference_hashes) and on the device."""
    import ctypes as C
    import test_oracle_paq8core as T
    from cmix_amd import build
    product = C.CDLL(build.build())
    proxy = _ProductAsOracle(product, O.lib())
    used = []
    orig = _ProductAsOracle.__getattr__

    def spy(self, name):
        if name.startswith("orc_p8_") and hasattr(self._p, "p8f_" + name[7:]):
            used.append(name)
        return orig(self, name)
    monkeypatch.setattr(_ProductAsOracle, "__getattr__", spy)
    monkeypatch.setattr(T.O, "lib", lambda: proxy)
    with O.scope():
        getattr(T, case)()
    assert used, "%s never called a product entry point" % case
