"""Child of tests/test_gpu_bgzf_write.py: bgzf.compress of every case of deflate_enc_cases at every level, in the given order,
in a process of its own (the library reads FX_DEBUG_FILL when it is loaded) -> a JSON file {"<case>/<level>": sha256 of the
stream, "__fill": [byte, blocks filled, bytes filled]}.

    python bgzf_write_child.py forward|reverse OUT.json"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main():
    order, out = sys.argv[1], sys.argv[2]
    import deflate_enc_cases
    from pyfastx_amd import _lib, bgzf
    cases = deflate_enc_cases.cases()
    keys = [(name, level) for name in cases for level in (0, 1, 2)]
    if order == "reverse":
        keys.reverse()
    res = {}
    for name, level in keys:
        res["%s/%d" % (name, level)] = hashlib.sha256(bgzf.compress(cases[name], level)).hexdigest()
    res["__fill"] = [int(v) for v in _lib.debug_fill_info()]
    with open(out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
