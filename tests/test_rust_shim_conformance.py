"""The Rust binding cannot be compiled here (no cargo), so what a compiler would check first is checked structurally: every trait the
shim implements — MachineProver, MachineProvingKey (crates/stark/src/prover.rs:30-199), ZKMProverComponents
(crates/prover/src/components.rs:6-26), the SDK's Prover (crates/sdk/src/provers/mod.rs:66-) — has all its required methods and
associated types defined in the `impl` block, with the reference's argument counts, and nothing the trait does not declare. The trait
shapes are data extracted from the reference by tests/golden/gen_rust_traits.py (names and counts, no source text)."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import gen_rust_traits as G  # noqa: E402

TRAITS = json.load(open(os.path.join(ROOT, "tests", "golden", "rust_traits.json")))


def impl_block(path, trait, for_type):
    src = open(os.path.join(ROOT, path)).read()
    src = re.sub(r"//[^\n]*", "", src)
    m = re.search(r"impl(<[^{]*?>)?\s+%s(<[^{]*?>)?\s+for\s+%s\b" % (trait, for_type), src)
    assert m, f"{path}: no `impl {trait} for {for_type}`"
    i = src.index("{", m.end())
    j = G.matching(src, i, "{", "}")
    body = src[i + 1:j]
    types = re.findall(r"^    type\s+(\w+)", body, flags=re.M)
    return types, {f["name"]: f for f in G.parse_fns(body)}


CASES = [
    ("MachineProver", "integration/zkm-hip/src/lib.rs", "HipProver"),
    ("MachineProvingKey", "integration/zkm-hip/src/lib.rs", "HipProvingKey"),
    ("ZKMProverComponents", "integration/sdk-hip/components.rs", "HipProverComponents"),
    ("Prover", "integration/sdk-hip/hip.rs", "HipProver"),
]


@pytest.mark.parametrize("trait,path,ty", CASES)
def test_impl_defines_what_the_reference_trait_requires(trait, path, ty):
    want = TRAITS[trait]
    types, fns = impl_block(path, trait, ty)
    assert sorted(types) == sorted(want["types"]), f"{path}: associated types {types} != {want['types']} ({want['file']}:{want['lines']})"
    declared = {f["name"]: f for f in want["fns"]}
    for name, f in declared.items():
        if not f["provided"]:
            assert name in fns, f"{path}: `impl {trait} for {ty}` lacks required fn {name} ({want['file']}:{want['lines'][0]}-{want['lines'][1]})"
    for name, f in fns.items():
        assert name in declared, f"{path}: fn {name} is not an item of trait {trait}"
        assert f["args"] == declared[name]["args"], f"{path}: fn {name} takes {f['args']} arguments, the trait declares {declared[name]['args']}"
        assert f["provided"], f"{path}: fn {name} has no body"


def test_the_golden_trait_shapes_are_the_reference_s():
    """The committed trait shapes are the ones tests/golden/gen_reference_tables.py extracted from the reference (their digest)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_reference_tables as GR
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_tables.json")))["rust_traits_sha256"]
    assert sorted(TRAITS) == sorted(name for name, _ in GR.TRAITS)
    assert GR.canonical_traits(TRAITS) == want
    req = [f["name"] for f in TRAITS["MachineProver"]["fns"] if not f["provided"]]
    assert req == ["new", "machine", "setup", "pk_from_vk", "pk_to_device", "pk_to_host", "commit", "open", "prove"]


def test_shim_points_at_files_that_exist():
    """Paths the Rust sources and INTEGRATION.md name inside this repository must exist (round 2 named a tool that did not)."""
    texts = [open(os.path.join(ROOT, p)).read() for p in
             ("integration/zkm-hip/src/lib.rs", "integration/zkm-hip/build.rs", "integration/sdk-hip/PATCHES.md", "INTEGRATION.md")]
    for t in texts:
        for m in re.finditer(r"\b((?:tools|ziren_amd|tests|integration|include|oracle)/[\w./-]+\.(?:py|rs|h|hpp|hip|cuh|json|md|c|sh))\b", t):
            p = m.group(1)
            if p.endswith("manifest.json"):   # a build product
                continue
            assert os.path.exists(os.path.join(ROOT, p)), f"named but missing: {p}"


def test_prove_mirrors_the_cpu_prover_s_order_of_calls():
    """prover.rs:660-693: dependencies, pk.observe_into, then per record generate_traces -> commit -> open on a clone of the challenger."""
    src = open(os.path.join(ROOT, "integration/zkm-hip/src/lib.rs")).read()
    body = src[src.index("fn prove("):]
    body = body[:body.index("\n    }\n") + 1]
    order = [body.index(s) for s in ("generate_dependencies(", "pk.observe_into(challenger)", "self.generate_traces(&record)",
                                     "self.commit(&record", "self.open(pk, shard_data, &mut challenger.clone())", "MachineProof { shard_proofs }")]
    assert order == sorted(order)
    assert "DebugConstraintBuilder" in body     # the where-bound of prover.rs:140-148
