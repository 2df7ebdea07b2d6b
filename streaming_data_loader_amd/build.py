"""Builds libsdl_batcher.so (HIP kernels + C ABI) in-tree for gfx950.

    python -m streaming_data_loader_amd.build      # or __graft_entry__.build()

Each translation unit is compiled with `hipcc --offload-arch=gfx950` into
build/, then linked into streaming_data_loader_amd/libsdl_batcher.so, which is
git-ignored but travels to the GPU box with the repo snapshot.  hipcc
cross-compiles without a GPU.
"""
import concurrent.futures as cf
import hashlib
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
BUILD = os.path.join(REPO, "build", "sdl")
LIB = os.path.join(PKG, "libsdl_batcher.so")
ARCH = os.environ.get("SDL_OFFLOAD_ARCH", "gfx950")

SOURCES = ["tokenize_wordpiece.hip", "tokenize_bpe.hip", "tokenize_unigram.hip", "pipeline.hip", "pack.hip", "pair.hip", "pair_mlm.hip", "json_text.hip", "transport_frame.hip", "inflate.hip", "zstd.hip",
           "assets.cpp", "sdl_batcher.cpp", "provider_json.cpp", "provider_gzip.cpp", "provider_zstd.cpp", "transport.cpp"]
HEADERS = ["common.hpp", "device_util.hpp", "kernels.hpp", "tok_device.hpp", "assets.hpp", "json.hpp", "unigram.hpp", "handle.hpp",
           "rows_device.hpp", "list_index.hpp", "mlm_pick.hpp", "span_noise.hpp", "pair_draw.hpp", "pack_queue.hpp", "wp_pack.hpp", "wp_extent.hpp", "wp_first.hpp", "zstd_format.hpp"]
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
         "-I", os.path.join(REPO, "include"), "-I", CSRC]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _newer(dst, srcs):
    if not os.path.exists(dst):
        return False
    t = os.path.getmtime(dst)
    return all(os.path.getmtime(s) <= t for s in srcs)


BUILD_ID_MARK = b"sdl-build-id:"


def source_hash(defines=()):
    """sha256 over the contents of every source, header and flag the library is
    built from -- what sdl_build_id() of an up-to-date library returns."""
    h = hashlib.sha256()
    for path in [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.join(REPO, "include", "sdl_batcher.h")]:
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS[:-4] + [f"-D{d}" for d in defines]).encode())
    return h.hexdigest()


def embedded_id(lib):
    """The build id compiled into a library file (read from its bytes, no dlopen), or None."""
    try:
        with open(lib, "rb") as f:
            data = f.read()
    except OSError:
        return None
    i = data.find(BUILD_ID_MARK)
    return data[i + len(BUILD_ID_MARK):i + len(BUILD_ID_MARK) + 64].decode("ascii", "replace") if i >= 0 else None


# The BertNormalizer settings beside bert-base-uncased's (cased, accent-keeping): their Unicode
# tables and the cased proxy vocabulary are committed once, under tests/golden/bert_normalizer/
# -- the one place of this repository that takes new binary files -- by
# tools/make_unicode_tables.py and tools/make_proxy_cased_assets.py, and the build installs
# them next to the library.  A tree without that directory builds as before and serves every
# tokenizer but those settings' (the loader names the missing table).
SETTINGS_SRC = os.path.join(REPO, "tests", "golden", "bert_normalizer")
SETTINGS_TABLES = ["bert_cased_unicode.bin", "bert_uncased_accents_unicode.bin", "bert_cased_stripped_unicode.bin"]
CASED_PROXY = os.path.join(PKG, "assets", "bert_cased_proxy")
CASED_VOCAB_GZ = os.path.join(SETTINGS_SRC, "bert_cased_proxy_vocab.txt.gz")


def cased_tokenizer_json(vocab):
    """What tokenizers' BertWordPieceTokenizer(vocab.txt, lowercase=False, strip_accents=False)
    saves: bert-base-cased's tokenizer.json layout around the vocabulary."""
    def added(i):
        return {"id": i, "content": vocab[i], "single_word": False, "lstrip": False, "rstrip": False,
                "normalized": False, "special": True}
    ids = {p: i for i, p in enumerate(vocab)}
    return {"version": "1.0", "truncation": None, "padding": None,
            "added_tokens": [added(ids[t]) for t in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")],
            "normalizer": {"type": "BertNormalizer", "clean_text": True, "handle_chinese_chars": True,
                           "strip_accents": False, "lowercase": False},
            "pre_tokenizer": {"type": "BertPreTokenizer"},
            "post_processor": {"type": "BertProcessing", "sep": ["[SEP]", ids["[SEP]"]], "cls": ["[CLS]", ids["[CLS]"]]},
            "decoder": {"type": "WordPiece", "prefix": "##", "cleanup": True},
            "model": {"type": "WordPiece", "unk_token": "[UNK]", "continuing_subword_prefix": "##",
                      "max_input_chars_per_word": 100, "vocab": ids}}


def install_assets():
    """Puts the tables of the other BertNormalizer settings into data/ and the cased proxy
    tokenizer (vocab.txt, tokenizer.json) into assets/bert_cased_proxy/ (git-ignored, like the
    library); files that are there with the right content are left alone."""
    import gzip
    import json

    if not os.path.isdir(SETTINGS_SRC):
        return

    def put(path, data):
        try:
            with open(path, "rb") as f:
                if f.read() == data:
                    return
        except OSError:
            pass
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, path)  # (several test processes may install at once)

    for name in SETTINGS_TABLES:
        with open(os.path.join(SETTINGS_SRC, name), "rb") as f:
            put(os.path.join(PKG, "data", name), f.read())
    with gzip.open(CASED_VOCAB_GZ, "rb") as f:
        text = f.read()
    put(os.path.join(CASED_PROXY, "vocab.txt"), text)
    vocab = text.decode("utf-8").split("\n")[:-1]
    put(os.path.join(CASED_PROXY, "tokenizer.json"),
        json.dumps(cased_tokenizer_json(vocab), ensure_ascii=False, indent=2).encode("utf-8"))


def build(verbose=False, force=False, jobs=4, defines=(), lib=None, build_dir=None):
    """defines: extra -D macros (diagnostic builds go to their own lib/build_dir).

    A library whose embedded build id equals source_hash() is used as is (the
    GPU box gets the library but not the objects: nothing is recompiled
    there); otherwise the changed objects are rebuilt and the id relinked."""
    install_assets()
    lib = lib or LIB
    bdir = build_dir or BUILD
    os.makedirs(bdir, exist_ok=True)
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    want = source_hash(defines)
    if not force and embedded_id(lib) == want:
        return lib
    hipcc = _hipcc()
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(REPO, "include", "sdl_batcher.h")]
    objs, todo = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(bdir, s + ".o")
        objs.append(obj)
        if force or not _newer(obj, [src] + hdrs):
            lang = ["-x", "hip"] if s.endswith(".hip") else []
            todo.append([hipcc] + FLAGS + [f"-D{d}" for d in defines] + lang + ["-c", src, "-o", obj])
    # the build id: a one-line translation unit regenerated per link
    idsrc = os.path.join(bdir, "build_id.cpp")
    with open(idsrc, "w") as f:
        f.write('extern "C" const char *sdl_build_id(void) {\n'
                f'    static const char id[] = "{BUILD_ID_MARK.decode()}{want}";\n'
                f'    return id + {len(BUILD_ID_MARK)};\n}}\n')
    idobj = idsrc + ".o"
    todo.append([hipcc, "-O2", "-fPIC", "-c", idsrc, "-o", idobj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"compile failed: {' '.join(cmd)}\n{p.stdout}\n{p.stderr}")
        return p.stderr

    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        for err in ex.map(run, todo):
            if verbose and err:
                print(err, file=sys.stderr)
    run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", lib] + objs + [idobj, "-ldl"])
    if embedded_id(lib) != want:
        raise RuntimeError(f"{lib}: build id not embedded")
    return lib


def build_stamps():
    """Diagnostic build with per-phase s_memtime stamps -> var/stamps/libsdl_batcher.so (travels to the GPU box)."""
    return build(defines=("SDL_STAMPS=1",), lib=os.path.join(REPO, "var", "stamps", "libsdl_batcher.so"),
                 build_dir=os.path.join(REPO, "build", "stamps"))


GZ256_LIB = os.path.join(REPO, "var", "gz256", "libsdl_batcher.so")


def build_gz256():
    """Diagnostic build whose inflate output batch (256 B) cannot hold a 258-byte match, the
    r02 hang: the decoder must leave through its no-progress exit (GZ_E_STALL) instead ->
    var/gz256/libsdl_batcher.so (tests/test_inflate_fuzz.py::test_device_no_progress_exit)."""
    return build(defines=("SDL_GZ_OBUF=256", "SDL_GZ_ALLOW_SMALL_OBUF"), lib=GZ256_LIB,
                 build_dir=os.path.join(REPO, "build", "var", "gz256", "obj"))


def build_ablations(levels=(3,)):
    """Diagnostic load-only build of the WordPiece chunk kernel (SDL_ABLATE: the window and
    record bits staged, nothing tokenized) -> var/abl3/libsdl_batcher.so (tools/pmc_calibration.py)."""
    return [build(defines=(f"SDL_ABLATE={n}",), lib=os.path.join(REPO, "var", f"abl{n}", "libsdl_batcher.so"),
                  build_dir=os.path.join(REPO, "build", f"abl{n}")) for n in levels]


def build_span_ablations(levels=(1, 2)):
    """Diagnostic builds of k_rows_span_t5 (SDL_SPAN_T5_ABLATE: 1 no Philox, 2 no selection either;
    their rows are not the contract's) -> var/span_abl{n}/libsdl_batcher.so, for
    SDL_LIB=... tools/span_policy_bench.py (where the policy's rows stage spends its time)."""
    return [build(defines=(f"SDL_SPAN_T5_ABLATE={n}",), lib=os.path.join(REPO, "var", f"span_abl{n}", "libsdl_batcher.so"),
                  build_dir=os.path.join(REPO, "build", f"span_abl{n}")) for n in levels]


if __name__ == "__main__":
    print(build(verbose="-v" in sys.argv, force="-f" in sys.argv))
