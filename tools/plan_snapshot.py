"""What the host queries answer for a matrix of configurations, digested: tests/golden/plan_tables.json is this tool's output
on the commit BEFORE the topology table was extracted, and tests/test_plan_tables_host.py recomputes it on the current build.

    python tools/plan_snapshot.py --write tests/golden/plan_tables.json     # the golden file (only ever from that parent)
    python tools/plan_snapshot.py --dump /tmp/records.txt [--set NAME]      # every record as a line, to diff two builds

A record is one line: the configuration, then ursn_query's return code, error text and sizes, a SHA-256 over the
ursn_query_layer rows, the ursn_query_concat pairs and ursn_bn_moving_size.  A refused call is recorded as !<rc>:<text>.  The
golden file keeps one SHA-256 per group of records (precision / ndim / max_batch / trainable), not the records.

The plans read their switches at create, so every switch set runs in a child process of its own (--child NAME).
"""
import argparse
import ctypes
import hashlib
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the matrix of tests/test_model_shapes_host.py (its accepted and its refused cases), 32 per axis
NDIMS = (2, 3)
CINS = (1, 2, 3, 4, 8)
WIDTHS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)
CLASSES = (1, 2, 3, 4, 6, 7, 8, 9)
STRIDES = (1, 3, 5)
PRECS = ("fp32", "bf16")
MAX_BATCH = (1, 2, 4)
TRAINABLE = (0, 1)
BENCH_STRIDES = 5   # bench.py constructs its workloads with the default num_strides

SWITCH_SETS = {
    "default": {},
    "split_cat0": {"URSN_SPLIT_CAT": "0"},
    "norm_on_load0": {"URSN_NORM_ON_LOAD": "0"},
    "norm_on_load2": {"URSN_NORM_ON_LOAD": "2"},
    "relu_mask0": {"URSN_RELU_MASK": "0"},
    "bf16_skip0_own0": {"URSN_BF16_SKIP0_OWN": "0"},
    "bf16_skip0_merge0": {"URSN_BF16_SKIP0_MERGE": "0"},
    "bf16_norm_on_load0": {"URSN_BF16_NORM_ON_LOAD": "0"},
    "bf16_relu_mask0": {"URSN_BF16_RELU_MASK": "0"},
    "bf16_scalar_in0": {"URSN_BF16_SCALAR_IN": "0"},
}


def bench_workloads():
    import bench
    return bench.WORKLOADS


def cases():
    """(group, (spatial, cin, F, ncls, ns, prec, max_batch, trainable)) for the whole matrix, in a fixed order."""
    for prec, ndim, mb, tr in itertools.product(PRECS, NDIMS, MAX_BATCH, TRAINABLE):
        group = "%s/ndim%d/mb%d/tr%d" % (prec, ndim, mb, tr)
        for cin, F, ncls, ns in itertools.product(CINS, WIDTHS, CLASSES, STRIDES):
            yield group, ((32,) * ndim, cin, F, ncls, ns, prec, mb, tr)
    for name, (dims, F, ncls, batch, _gen) in sorted(bench_workloads().items()):
        prec = "bf16" if name.endswith("_bf16") else "fp32"
        for mb, tr in itertools.product(sorted(set(MAX_BATCH + (batch,))), TRAINABLE):
            yield "bench/mb%d/tr%d" % (mb, tr), (tuple(dims[:-1]), dims[-1], F, ncls, BENCH_STRIDES, prec, mb, tr)


def make_config(_lib, case):
    spatial, cin, F, ncls, ns, prec, mb, tr = case
    cfg = _lib.ursn_config()
    cfg.ndim = len(spatial)
    for i in range(3):
        cfg.spatial[i] = spatial[i] if i < len(spatial) else 1
    cfg.cin, cfg.base_filters, cfg.num_class, cfg.num_strides = cin, F, ncls, ns
    cfg.max_batch, cfg.trainable, cfg.use_weight, cfg.bn_eps = mb, tr, 1, 1e-3
    cfg.act_dtype = 1 if prec == "bf16" else 0
    return cfg


def _refused(lib, rc):
    return "!%d:%s" % (rc, (lib.ursn_last_error() or b"").decode("utf-8", "replace"))


def layer_rows(_lib, lib, cfg, n_layers):
    """The ursn_query_layer rows of an accepted configuration (and the refusal one past the end), or the refusal of row 0."""
    info = _lib.ursn_layer_info()
    rows = []
    for i in range(n_layers + 1):
        rc = lib.ursn_query_layer(ctypes.byref(cfg), i, ctypes.byref(info))
        if rc != 0:
            rows.append(_refused(lib, rc))
            break
        rows.append((info.name.decode(), info.transposed, info.k, info.stride, info.cin, info.cout, info.relu, info.w_offset,
                     info.beta_offset))
    return rows


def concat_pairs(lib, cfg):
    """The ursn_query_concat pairs step by step up to the first refusal, which is recorded too."""
    first, second = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    pairs = []
    for step in range(9):
        rc = lib.ursn_query_concat(ctypes.byref(cfg), step, first, second, 128)
        if rc != 0:
            pairs.append(_refused(lib, rc))
            break
        pairs.append((first.value.decode(), second.value.decode()))
    return pairs


def record(_lib, lib, case):
    """One configuration's answers as a dict; layers / concat are the tables themselves (line() digests them)."""
    cfg = make_config(_lib, case)
    sizes = _lib.ursn_sizes()
    rc = lib.ursn_query(ctypes.byref(cfg), ctypes.byref(sizes))
    out = {"case": case, "rc": rc, "error": _refused(lib, rc) if rc else ""}
    out["sizes"] = (sizes.n_params, sizes.n_layers, sizes.n_tensors, sizes.workspace_bytes) if rc == 0 else None
    out["layers"] = layer_rows(_lib, lib, cfg, int(sizes.n_layers) if rc == 0 else 0)
    out["concat"] = concat_pairs(lib, cfg)
    total = ctypes.c_int64(0)
    rc2 = lib.ursn_bn_moving_size(ctypes.byref(cfg), ctypes.byref(total))
    out["bn_moving"] = total.value if rc2 == 0 else _refused(lib, rc2)
    return out


def line(rec):
    sha = hashlib.sha256(repr(rec["layers"]).encode()).hexdigest()
    return "%r|%d|%s|%r|%s|%r|%r" % (rec["case"], rec["rc"], rec["error"], rec["sizes"], sha, rec["concat"], rec["bn_moving"])


def run_here(dump=None):
    """The digest of every group under this process's environment: {group: {n, accepted, sha256}}."""
    from uresnet_amd import _lib
    lib = _lib.load()
    groups = {}
    for group, case in cases():
        rec = record(_lib, lib, case)
        g = groups.setdefault(group, {"n": 0, "accepted": 0, "h": hashlib.sha256()})
        text = line(rec)
        g["n"] += 1
        g["accepted"] += rec["rc"] == 0
        g["h"].update(text.encode() + b"\n")
        if dump is not None:
            dump.write(group + "|" + text + "\n")
    return {k: {"n": g["n"], "accepted": g["accepted"], "sha256": g["h"].hexdigest()} for k, g in groups.items()}


def child_env(name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("URSN_")}
    env.update(SWITCH_SETS[name])
    return env


def run_sets(names=None):
    """Every switch set in a child of its own, all at once (host work only: no child touches a device)."""
    names = list(names or SWITCH_SETS)
    procs = [(n, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", n], env=child_env(n),
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for n in names]
    out = {}
    for n, p in procs:
        so, se = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("plan_snapshot child %s failed (%d):\n%s" % (n, p.returncode, se[-4000:]))
        out[n] = json.loads(so.strip().splitlines()[-1])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", metavar="JSON", help="write the golden file (run this on the parent commit only)")
    ap.add_argument("--parent", default="", help="the commit the golden file is taken from (recorded in it)")
    ap.add_argument("--dump", metavar="FILE", help="write every record of one switch set as a line")
    ap.add_argument("--set", default="default", choices=sorted(SWITCH_SETS))
    ap.add_argument("--child", choices=sorted(SWITCH_SETS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(run_here()))
        return
    if args.dump:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump-here", args.dump], env=child_env(args.set))
        sys.exit(p.returncode)
    sets = run_sets()
    doc = {"parent": args.parent, "sets": sets}
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    if args.write:
        with open(args.write, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump-here":
        with open(sys.argv[2], "w") as f:
            run_here(f)
    else:
        main()
