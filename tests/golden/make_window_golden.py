"""Writes tests/golden/window_v1.npz: inputs and expected outputs of rdf_window for four cases of 1000 to 1500 rows
(not the few thousand one would like: the archive has to stay below mixed_batches.arrow's 100 KiB, and the eight
expected outputs per case — every function is frozen for every case — are most of its bytes), so that the
GPU box compares against bytes generated where pandas could check the reference (tests/test_window_ref.py).

    python tests/golden/make_window_golden.py            # rewrites the fixture next to this file

Layout of the archive: "meta" is a JSON string {case: {"partition": [key...], "order": [key...], "calls": [[name, param]...]}}
with key = {"kind": "num" | "utf8", "desc": bool}; the arrays are "<case>/<p|o><i>/values" (+ "/valid") for numeric keys,
"<case>/<p|o><i>/offsets", "/data" (+ "/valid") for Utf8 keys, and "<case>/out<c>" (+ "/valid" for lag / lead).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import window_ref  # noqa: E402

CALLS = [["row_number", 0], ["rank", 0], ["dense_rank", 0], ["percent_rank", 0], ["cume_dist", 0], ["ntile", 7], ["lag", 1], ["lead", 3]]
CITIES = [b"Aberdeen", b"Bath", b"Birmingham", b"Bradford", b"Brighton", b"Bristol", b"Cambridge", b"Cardiff", b"", b"Bath\0",
          b"Bat", b"York", b"Z\xc3\xbcrich", b"Bristol Temple Meads"]


def float_specials(rng, n, dtype=np.float64):
    v = np.round(rng.normal(size=n) * 3).astype(dtype)
    u = np.uint64 if dtype == np.float64 else np.uint32
    nan_pos = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64)
    if dtype == np.float32:
        nan_pos = np.array([0x7FC00000, 0x7FC00001, 0x7F800001, 0x7FFFFFFF], dtype=np.uint64)
    sign = np.uint64(1) << np.uint64(8 * np.dtype(dtype).itemsize - 1)
    pats = np.concatenate([nan_pos, nan_pos | sign]).astype(u).view(dtype)
    pick = rng.random(n)
    v[pick < 0.05] = pats[rng.integers(0, len(pats), int((pick < 0.05).sum()))]
    v[(pick >= 0.05) & (pick < 0.10)] = -0.0
    v[(pick >= 0.10) & (pick < 0.15)] = 0.0
    v[(pick >= 0.15) & (pick < 0.17)] = np.inf
    v[(pick >= 0.17) & (pick < 0.19)] = -np.inf
    return v


def num_key(values, valid=None, desc=False):
    return {"kind": "num", "desc": desc, "values": values, "valid": valid}


def utf8_key(rows, desc=False):
    return {"kind": "utf8", "desc": desc, "rows": rows}


def build_cases():
    cases = {}
    rng = np.random.default_rng(20240601)
    n = 1500
    cases["mixed_numeric"] = {
        "partition": [num_key(rng.integers(-3, 3, n).astype(np.int32)),
                      num_key(rng.integers(0, 4, n).astype(np.int16), rng.random(n) > 0.1)],
        "order": [num_key(float_specials(rng, n)), num_key(rng.integers(0, 5, n).astype(np.int64), rng.random(n) > 0.1, desc=True)],
    }
    rng = np.random.default_rng(20240602)
    n = 1200
    rows = [None if rng.random() < 0.05 else CITIES[int(rng.integers(0, len(CITIES)))] for _ in range(n)]
    cases["text_partition"] = {
        "partition": [utf8_key(rows)],
        "order": [num_key(float_specials(rng, n, np.float32), rng.random(n) > 0.1, desc=True)],
    }
    rng = np.random.default_rng(20240603)
    n = 1000
    prefix = bytes(rng.integers(97, 123, 1024, dtype=np.uint8))
    rows = [None if rng.random() < 0.1 else prefix[:int(rng.integers(1000, 1025))] + bytes(rng.integers(97, 99, int(rng.integers(0, 3)), dtype=np.uint8))
            for _ in range(n)]
    cases["text_order"] = {
        "partition": [],
        "order": [utf8_key(rows, desc=True), num_key(rng.integers(0, 3, n).astype(np.uint8))],
    }
    rng = np.random.default_rng(20240604)
    n = 1025
    cases["float_partition"] = {
        "partition": [num_key(float_specials(rng, n))],
        "order": [],
    }
    for c in cases.values():
        c["calls"] = CALLS
    return cases


def ref_key(k, with_desc):
    if k["kind"] == "num":
        return (k["values"], k["valid"], k["desc"]) if with_desc else (k["values"], k["valid"])
    return (k["rows"], None, k["desc"]) if with_desc else (k["rows"], None)


def expected(case):
    return window_ref.window_ref([ref_key(k, False) for k in case["partition"]], [ref_key(k, True) for k in case["order"]],
                                 [tuple(c) for c in case["calls"]])


def to_arrays(cases):
    arrays, meta = {}, {}
    for name, case in cases.items():
        meta[name] = {"partition": [], "order": [], "calls": case["calls"]}
        for kind, tag in (("partition", "p"), ("order", "o")):
            for i, k in enumerate(case[kind]):
                meta[name][kind].append({"kind": k["kind"], "desc": bool(k["desc"])})
                base = f"{name}/{tag}{i}"
                if k["kind"] == "num":
                    arrays[base + "/values"] = k["values"]
                    if k["valid"] is not None:
                        arrays[base + "/valid"] = np.asarray(k["valid"], dtype=bool)
                else:
                    rows = k["rows"]
                    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
                    arrays[base + "/offsets"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
                    arrays[base + "/data"] = np.frombuffer(b"".join(b"" if r is None else r for r in rows), dtype=np.uint8)
                    if any(r is None for r in rows):
                        arrays[base + "/valid"] = np.array([r is not None for r in rows], dtype=bool)
        for c, out in enumerate(expected(case)):
            if isinstance(out, tuple):
                arrays[f"{name}/out{c}"], arrays[f"{name}/out{c}/valid"] = out
            else:
                arrays[f"{name}/out{c}"] = out
    arrays["meta"] = np.array(json.dumps(meta))
    return arrays


def load(path):
    """-> {case: {"partition": [key...], "order": [key...], "calls": [(name, param)...], "expected": [...]}} with the keys in
    build_cases()' form."""
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    cases = {}
    for name, m in meta.items():
        case = {"calls": [tuple(c) for c in m["calls"]], "expected": []}
        for kind, tag in (("partition", "p"), ("order", "o")):
            case[kind] = []
            for i, k in enumerate(m[kind]):
                base = f"{name}/{tag}{i}"
                valid = z[base + "/valid"] if base + "/valid" in z.files else None
                if k["kind"] == "num":
                    case[kind].append(num_key(z[base + "/values"], valid, k["desc"]))
                else:
                    offs, data = z[base + "/offsets"], z[base + "/data"].tobytes()
                    rows = [data[offs[j]:offs[j + 1]] if valid is None or valid[j] else None for j in range(len(offs) - 1)]
                    case[kind].append(utf8_key(rows, k["desc"]))
        for c, (fn, _p) in enumerate(case["calls"]):
            out = z[f"{name}/out{c}"]
            case["expected"].append((out, z[f"{name}/out{c}/valid"]) if fn in ("lag", "lead") else out)
        cases[name] = case
    return cases


if __name__ == "__main__":
    path = os.path.join(HERE, "window_v1.npz")
    np.savez_compressed(path, **to_arrays(build_cases()))
    print(path, os.path.getsize(path), "bytes")
