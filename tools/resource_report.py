#!/usr/bin/env python3
"""Per-kernel resource report of two builds of the same kernel files, side by side
(profiles/hash_vocab_resources.json).  For each build and each TU, compile with the flags of
build.py plus `--cuda-device-only -S -Rpass-analysis=kernel-resource-usage` to DIR/<tu>.s and keep
the compiler's stderr as DIR/<tu>.remarks; then
    python tools/resource_report.py PARENT_DIR NEW_DIR out.json sha handshake duplex duplex_split
Exit status 1 when a kernel misses a condition: LDS equal, occupancy not lower, scratch not higher,
total and VALU instruction counts within 0.5 %."""
import json
import re
import subprocess
import sys

FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}


def remarks(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None and k in FIELDS:
            cur[FIELDS[k]] = int(v)
    return out


def counts(path, names):
    out, cur = {}, None
    for line in open(path):
        s = line.split(";")[0].strip()
        if cur is None:
            if s.endswith(":") and s[:-1] in names:
                cur = s[:-1]
                out[cur] = [0, 0]
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if not s or s[0] == "." or s.endswith(":"):
            continue
        out[cur][0] += 1
        if s.startswith("v_"):
            out[cur][1] += 1
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.split("\n")))


def main(pdir, ndir, tus, dst):
    rows, bad = [], 0
    for tu in tus:
        pr, nr = remarks(f"{pdir}/{tu}.remarks"), remarks(f"{ndir}/{tu}.remarks")
        pc, nc = counts(f"{pdir}/{tu}.s", set(pr)), counts(f"{ndir}/{tu}.s", set(nr))
        dm = demangle(sorted(set(pr) | set(nr)))
        for k in sorted(set(pr) | set(nr)):
            if k not in pr or k not in nr:
                rows.append({"tu": tu + ".hip", "kernel": dm[k], "ok": False, "note": "kernel set differs"})
                bad += 1
                continue
            p, n = dict(pr[k]), dict(nr[k])
            p["insts"], p["valu"] = pc[k]
            n["insts"], n["valu"] = nc[k]
            di = (n["insts"] - p["insts"]) / p["insts"]
            dv = (n["valu"] - p["valu"]) / p["valu"]
            ok = (n["lds"] == p["lds"] and n["occupancy"] >= p["occupancy"] and n["scratch"] <= p["scratch"]
                  and abs(di) <= 0.005 and abs(dv) <= 0.005)
            bad += not ok
            rows.append({"tu": tu + ".hip", "kernel": dm[k], "parent": p, "new": n,
                         "insts_delta_pct": round(100 * di, 3), "valu_delta_pct": round(100 * dv, 3), "ok": ok})
    doc = {"what": "hipcc --offload-arch=gfx950 -O3 -std=c++20 --cuda-device-only -S "
                   "-Rpass-analysis=kernel-resource-usage, parent commit vs this tree; insts / valu are "
                   "instruction lines of the kernel's disassembly (valu: v_*); scratch is bytes per lane",
           "conditions": "lds equal; occupancy not lower; scratch not higher; insts and valu within 0.5 %",
           "all_ok": bad == 0, "kernels": rows}
    with open(dst, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in rows:
        if "parent" not in r:
            print("MISSING", r["kernel"])
            continue
        p, n = r["parent"], r["new"]
        print(f'{"ok " if r["ok"] else "BAD"} {r["kernel"][:70]:70s} vgpr {p["vgprs"]}->{n["vgprs"]} scr {p["scratch"]}->{n["scratch"]} '
              f'occ {p["occupancy"]}->{n["occupancy"]} lds {p["lds"]}->{n["lds"]} insts {p["insts"]}->{n["insts"]} valu {p["valu"]}->{n["valu"]}')
    return bad


if __name__ == "__main__":
    sys.exit(1 if main(sys.argv[1], sys.argv[2], sys.argv[4:], sys.argv[3]) else 0)
