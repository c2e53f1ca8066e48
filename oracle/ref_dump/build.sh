#!/bin/bash
# Builds oracle/_ref/ref_dump from the real reference sources; records the outcome in oracle/_ref/STATUS and which
# Eigen / ifopt were used (system packages, or the subset under oracle/ref_dump/subset) in oracle/_ref/DEPS.
# Where the reference sources are absent but a built oracle/_ref/ref_dump arrived with the tree, both are left alone.
# Where they are present, anything but "available" is a defect of the recipe, the subset or the driver: the logs of the
# failed attempt stay in oracle/_ref/configure.log and build.log.
set -u
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$(mkdir -p "$HERE/../_ref" && cd "$HERE/../_ref" && pwd)
REF=${TOWR_REFERENCE_DIR:-/root/reference/towr}
ROOT=$(cd "$HERE/../.." && pwd)

if [ ! -d "$REF/src" ]; then
  if [ -x "$OUT/ref_dump" ] && [ -f "$OUT/STATUS" ]; then
    echo "reference sources not present at $REF: keeping the ref_dump that is here ($(cat "$OUT/STATUS"))"
    exit 0
  fi
  echo "unavailable: reference sources not present at $REF" > "$OUT/STATUS"
else
  # The build tree is oracle/_ref/cmake and is removed again after a successful build: a CMake cache is tied to the paths
  # it was made with, so a tree left behind is refused once the repository is moved or copied (and an older recipe
  # configured oracle/_ref/build for another CMakeLists.txt).  One left by a failed build is reused only if it was made
  # for this source directory at this path.
  BUILD=$OUT/cmake
  if [ -f "$BUILD/CMakeCache.txt" ] && ! { grep -qxF "CMAKE_HOME_DIRECTORY:INTERNAL=$HERE" "$BUILD/CMakeCache.txt" \
       && grep -qxF "CMAKE_CACHEFILE_DIR:INTERNAL=$BUILD" "$BUILD/CMakeCache.txt"; }; then
    rm -rf "$BUILD"
  fi
  rm -f "$OUT/configure.log" "$OUT/build.log"
  if mkdir -p "$BUILD" \
     && cmake -S "$HERE" -B "$BUILD" -DTOWR_REFERENCE_DIR="$REF" -DTOWR_AMD_ROOT="$ROOT" -DCMAKE_BUILD_TYPE=Release > "$OUT/configure.log" 2>&1 \
     && cmake --build "$BUILD" -j"${TWR_REF_BUILD_JOBS:-8}" > "$OUT/build.log" 2>&1 \
     && [ -x "$BUILD/ref_dump" ]; then
    cp "$BUILD/ref_dump" "$OUT/ref_dump.new" && mv "$OUT/ref_dump.new" "$OUT/ref_dump"
    cp "$BUILD/DEPS" "$OUT/DEPS"
    echo "available" > "$OUT/STATUS"
    rm -rf "$BUILD"
  else
    rm -f "$OUT/ref_dump"
    WHY=$(grep -m1 -hiE 'could not find|error' "$OUT/configure.log" "$OUT/build.log" 2>/dev/null | head -1 | cut -c1-200)
    [ -n "$WHY" ] || WHY=$(tail -qn1 "$OUT/configure.log" "$OUT/build.log" 2>/dev/null | tail -1 | cut -c1-200)
    echo "unavailable: the build failed (oracle/_ref/configure.log, build.log): $WHY" > "$OUT/STATUS"
  fi
fi
cat "$OUT/STATUS"
