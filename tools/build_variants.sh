# Build A/B library variants of the HIP decoder into qldpcsim_amd/_build/var_<name>.so
# usage: bash tools/build_variants.sh name1 "EXTRA FLAGS" [name2 "FLAGS" ...]
#        name "HEAD" as flags builds the committed sources (git HEAD) instead.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC="$ROOT/qldpcsim_amd/csrc"
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  # a variant is built from nothing: its library and every per-unit object of
  # its name (the Makefile's UNITS) go first, since make compares mtimes only
  # and neither new flags nor archived sources (old mtimes) would rebuild them
  make -s -C "$CSRC" LIB=var_$name.so clean-lib
  if [ "$flags" = "HEAD" ]; then
    tmp=$(mktemp -d)
    (cd "$ROOT" && git archive HEAD qldpcsim_amd/csrc include) | tar -x -C "$tmp"
    make -s -C "$tmp/qldpcsim_amd/csrc" OUT_DIR="$ROOT/qldpcsim_amd/_build" LIB=var_$name.so 2>&1 | grep -i error || true
    rm -rf "$tmp"
  else
    make -s -C "$CSRC" LIB=var_$name.so EXTRA="-DQLDPC_EXPERIMENTS $flags" 2>&1 | grep -i error || true
  fi
  ls -la "$ROOT/qldpcsim_amd/_build/var_$name.so"
done
