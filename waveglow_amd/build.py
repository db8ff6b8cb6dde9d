"""Build libwaveglow_amd.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

``python -m waveglow_amd.build [-o OUT.so] [-DFLAG ...]`` builds a variant library (diagnostic builds such as
-DWG_STAMPS) beside the in-tree one; load it with WAVEGLOW_AMD_LIB=OUT.so.  `-m` imports the whole package first, and
waveglow_amd._lib fixes the library path at that import: a tool that builds a variant and then loads it does the build in a
child process and sets WAVEGLOW_AMD_LIB before its own first import of the package (tools/stamp_phases.py)."""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB = os.path.join(CSRC, "libwaveglow_amd.so")
SOURCES = ["kernels.hip", "stft.hip", "stft_loss.hip", "train.hip", "train_prep.hip", "wav.hip", "metrics.hip", "data.hip", "api.cpp", "stft_api.cpp", "train_api.cpp", "metrics_api.cpp",
           "data_api.cpp", "pitch.hip", "pitch_api.cpp", "resample.hip", "resample_grad.hip", "resample_api.cpp", "stoi.hip", "stoi_grad.hip", "stoi_api.cpp",
           "likelihood.hip", "likelihood_api.cpp", "softdtw.hip", "softdtw_api.cpp", "mel_loss.hip", "mel_loss_api.cpp", "stream.hip", "stream_api.cpp"]
HEADERS = ["wg_plan.h", "wg_stream.h", "wg_stftconv.h", "wg_melloss.h","wg_softdtw.h", "wg_likelihood.h","wg_common.h", "wg_train.h", "wg_host.h", "wg_stft.h", "wg_metrics.h", "wg_pitch.h", "wg_resample.h", "wg_stoi.h", os.path.join("..", "..", "include", "waveglow_amd.h")]


def _hipcc() -> str:
  for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
    if cand and os.path.isfile(cand):
      return cand
  raise RuntimeError("hipcc not found")


def needs_build() -> bool:
  if not os.path.isfile(LIB):
    return True
  t = os.path.getmtime(LIB)
  return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def build_library(force: bool = False, verbose: bool = False, extra_flags=(), out: str | None = None) -> str:
  """hipcc -> in-tree .so, or with `extra_flags` / `out` a variant library at `out` (always built; `out` is required with
  extra flags so that a variant never replaces the in-tree library).  The build FAILS if any kernel spills registers or uses scratch: the WN-layer
  kernel issues loads from inline asm with hand-counted waits, and a compiler spill of such a register
  (a scratch store before the data has landed) would silently corrupt results."""
  if extra_flags and not out:
    raise ValueError("a build with extra flags needs an output path of its own")
  if not out and not force and not needs_build():
    return LIB
  lib = os.path.abspath(out) if out else LIB
  cmd = [_hipcc(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value",
         "-Rpass-analysis=kernel-resource-usage", *extra_flags, "-o", lib + ".tmp"] + SOURCES
  res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
  if res.returncode != 0:
    raise RuntimeError("hipcc failed:\n" + res.stderr)
  report, name = [], None
  for line in res.stderr.splitlines():
    if "Function Name:" in line:
      name = line.split("Function Name:")[1].split("[")[0].strip()
    # SGPR spills go to VGPR lanes (v_writelane), never to memory: tolerated.  VGPR spills / scratch are not.
    for key in ("VGPRs Spill:", "ScratchSize [bytes/lane]:"):
      if key in line and name:
        val = int(line.split(key)[1].split("[")[0].strip())
        if val != 0:
          report.append(f"{name}: {key} {val}")
  if verbose:
    print(res.stderr)
  if report:
    os.remove(lib + ".tmp")
    raise RuntimeError("register spills / scratch in device code (forbidden, see build_library doc):\n  " + "\n  ".join(report))
  os.replace(lib + ".tmp", lib)
  return lib


if __name__ == "__main__":
  import argparse
  ap = argparse.ArgumentParser(description=__doc__)
  ap.add_argument("-o", "--out", help="output library (default: the in-tree library, rebuilt only when stale)")
  ap.add_argument("-v", "--verbose", action="store_true", help="print the compiler's resource-usage report")
  args, flags = ap.parse_known_args()      # everything else (-D..., -U...) goes to hipcc
  print(build_library(force=bool(args.out), verbose=args.verbose, extra_flags=flags, out=args.out))
