#!/bin/bash
# build_variant.sh NAME [extra hipcc flags...] : full library build with extra -D flags -> tools/ablate/variants/NAME.so
# The compiler, the source list and the per-file flags come from transformer4sed_amd/build.py (_hipcc, SOURCES, FLAGS, FILE_FLAGS), so a variant
# exports the same symbols as the library and _lib accepts it through SED_HIP_LIB.
set -e
cd "$(dirname "$0")/../.."
name=$1; shift
out=tools/ablate/variants/$name.so
obj=$(mktemp -d)
trap 'rm -rf "$obj"' EXIT
mkdir -p tools/ablate/variants
# first line: the compiler; then one line per source: "<file> <flags...>"
mapfile -t jobs < <(python3 -c '
import importlib.util, shlex
spec = importlib.util.spec_from_file_location("b", "transformer4sed_amd/build.py")
b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
print(b._hipcc())
for s in b.SOURCES:
    print(s, shlex.join(b.FLAGS + b.FILE_FLAGS.get(s, [])))
')
hipcc=${jobs[0]}
pids=()
for j in "${jobs[@]:1}"; do
  read -r f ff <<< "$j"
  $hipcc $ff "$@" -c transformer4sed_amd/csrc/$f -o "$obj/${f%.hip}.o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
$hipcc --offload-arch=gfx950 -shared -fPIC "$obj"/*.o -o $out
echo built $out
