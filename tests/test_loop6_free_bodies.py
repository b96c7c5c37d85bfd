"""The two loop bodies of the huge geometry (tools/gen_v6_loop_asm.py): the committed header is what the generator prints, and the test-free
bodies the build generates (--free) run the SAME MFMAs on the same operands, LDS-DMA pieces, fragment reads and one barrier per half-tile
as the tested ones -- and none of the test's instructions."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "gen_v6_loop_asm.py")


def generate(*args):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("V5_", "V6_"))}
    return subprocess.run([sys.executable, GEN, *args], check=True, capture_output=True, text=True, env=env).stdout


def loop_bodies(text, struct):
    """{(D, UB): the asm lines between the loop's entry label and its back branch}"""
    out = {}
    for m in re.finditer(r"struct %s<(\d+), (\d+)> \{(.*?)\n\};" % struct, text, re.S):
        lines = re.findall(r'^\s*"(.*?)\\n\\t"$', m.group(3), re.M)
        out[(int(m.group(1)), int(m.group(2)))] = lines[lines.index("20:"):lines.index("s_branch 20b")]
    return out


def test_committed_header_is_the_generators_output():
    with open(os.path.join(ROOT, "pda_amd", "csrc", "pda_v6_loop_asm.h")) as f:
        assert f.read() == generate()


def test_free_bodies_keep_the_mfmas_and_the_memory_operations_and_drop_the_tests():
    tested, free = loop_bodies(generate(), "Loop6"), loop_bodies(generate("--free"), "Loop6Free")
    assert sorted(tested) == sorted(free) == [(64, 8), (64, 16), (128, 8), (128, 16), (256, 8)]
    pick = lambda lines, pat: [l for l in lines if re.match(pat, l)]
    for inst in tested:
        t, f = tested[inst], free[inst]
        d, ub = inst
        mf = pick(t, "v_mfma")
        assert len(mf) == 2 * 2 * ub * (d // 32) and pick(f, "v_mfma") == mf, inst            # 32 x NK MFMAs per half-tile at UB = 16, same operands, same order
        assert pick(f, "ds_read_b128") == pick(t, "ds_read_b128"), inst                      # the fragment reads
        rows = lambda lines: [l for l in pick(lines, "global_load_lds") if "s[84:85]" in l]
        assert rows(f) == rows(t) and len(pick(f, "global_load_lds")) == len(rows(f)), inst   # the row pieces; no meta entry
        assert len(pick(f, "s_barrier")) == len(pick(t, "s_barrier")) == 2, inst             # one per half-tile
        for gone in ("v_max", "v_cmp", "s_or_b64", "ds_max_u32", "ds_read_b32", "ds_read_b64", "v_fma", "v_readfirstlane"):
            assert pick(t, gone) and not pick(f, gone), (inst, gone)
