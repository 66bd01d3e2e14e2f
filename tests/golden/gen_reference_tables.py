#!/usr/bin/env python3
"""Extract, as data, what the tests once read from a checkout of the reference at run time, so that they run without one:

    core_maximal_shapes   crates/core/machine/src/shape/maximal_shapes.json: the sizes, the number of shapes per size and a sha256
                          over the table in canonical form (`canonical_shapes`; the file itself is 2 MB)
    recursion_shapes      RecursionShapeConfig::default and REDUCE_BATCH_SIZE (gen_recursion_shapes.extract)
    weierstrass_moduli    the base-field modulus of every curve of crates/curves/src/weierstrass, as hex
    rust_traits_sha256    a sha256 over the trait shapes gen_rust_traits.py extracts, in canonical form (`canonical_traits`)

Output: tests/golden/reference_tables.json — numbers, names and digests only. Run where a checkout of the reference is (its root in
$ZKM_REFERENCE or as the first argument); the output is committed."""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_tables.json")
CURVES = (("Secp256k1", "secp256k1"), ("Secp256r1", "secp256r1"), ("Bn254", "bn254"), ("Bls12381", "bls12_381"))
TRAITS = (("MachineProver", "crates/stark/src/prover.rs"), ("MachineProvingKey", "crates/stark/src/prover.rs"),
          ("ZKMProverComponents", "crates/prover/src/components.rs"), ("Prover", "crates/sdk/src/provers/mod.rs"))


def canonical_shapes(table):
    """sha256 of {"<log2 shard size>": [{chip: log2 height}, ...]} as sorted-key compact JSON (shape order kept: it is the table's)."""
    return hashlib.sha256(json.dumps(table, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def canonical_traits(traits):
    return hashlib.sha256(json.dumps(traits, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ZKM_REFERENCE"]
    sys.path.insert(0, HERE)
    import gen_recursion_shapes
    import gen_rust_traits
    src = json.load(open(os.path.join(ref, "crates/core/machine/src/shape/maximal_shapes.json")))
    table = {k: [s["inner"] for s in lst] for k, lst in src.items()}
    moduli = {}
    for curve, fname in CURVES:
        text = open(os.path.join(ref, "crates/curves/src/weierstrass", fname + ".rs")).read()
        m = re.search(r"const MODULUS: &'static \[u8\] = &\[(.*?)\];", text, re.S)
        moduli[curve] = hex(int.from_bytes(bytes(int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(1))), "little"))
    gen_rust_traits.REF = ref
    traits = {name: gen_rust_traits.parse_trait(path, name) for name, path in TRAITS}
    out = {"generated_by": "tests/golden/gen_reference_tables.py",
           "core_maximal_shapes": {"sizes": sorted(int(k) for k in table), "counts": {k: len(v) for k, v in sorted(table.items())},
                                   "sha256": canonical_shapes(table)},
           "recursion_shapes": gen_recursion_shapes.extract(ref),
           "weierstrass_moduli": moduli,
           "rust_traits_sha256": canonical_traits(traits)}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
