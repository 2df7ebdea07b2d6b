"""Writes tests/golden/zstd/*.zst and manifest.json: frames made by the libzstd copies found on this
machine (through ctypes, loaded by path) and by the pure-Python writer of tests/zstd_cases.py.

    python tests/golden/make_zstd_fixtures.py

Every frame is decoded again with libzstd before it is written; the modes in the manifest are what
the header walker finds in the bytes."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zstd_cases as zc  # noqa: E402


def main():
    libs = zc.find_libzstd()
    if not libs:
        raise SystemExit("no libzstd found")
    old, new = libs[0], libs[-1]
    os.makedirs(zc.ZDIR, exist_ok=True)
    for f in os.listdir(zc.ZDIR):
        if f.endswith(".zst"):
            os.remove(os.path.join(zc.ZDIR, f))
    entries = []

    def add(name, z, plain, recipe, encoder, extra=()):
        assert old.decompress(z, len(plain)) == plain, name
        assert len(z) < 400 << 10, (name, len(z))
        with open(os.path.join(zc.ZDIR, name + ".zst"), "wb") as f:
            f.write(z)
        entries.append({"name": name, "file": name + ".zst", "recipe": recipe, "plain_len": len(plain),
                        "sha256": zc.sha256(plain), "encoder": encoder, "modes": sorted(zc.modes_of(z)),
                        "extra": sorted(extra)})

    for name, rec, enc in zc.LIB_RECIPES:
        plain = zc.plaintext(rec)
        add(name, zc.lib_compress(old, plain, enc), plain, dict(rec, enc=enc), "libzstd " + old.version)
        if new.version != old.version and name in zc.NEWER_RECIPES:
            add(name + "_new", zc.lib_compress(new, plain, enc), plain, dict(rec, enc=enc), "libzstd " + new.version)
    for name, z, plain, extra in zc.written_frames():
        add(name, z, plain, {"plain": "written"}, "tests/zstd_cases.py writer", extra)
    total = sum(os.path.getsize(os.path.join(zc.ZDIR, e["file"])) for e in entries)
    assert total < 2 << 20, total
    with open(zc.MANIFEST, "w") as f:
        json.dump({"fixtures": entries}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(entries)} fixtures, {total} bytes")


if __name__ == "__main__":
    main()
