# One kernel file rebuilt with extra flags for a measurement: `[SRC=vt] bash tools/build_variant.sh NAME FLAG ...`
# compiles track.hip (or $SRC.hip) with the extra flags, links it with the product's other objects
# (../build/*.o, `make` first) into tools/probe_lib/libgnss_NAME.so. Load with GNSS_LIB=<path>
# (tools/gpu.sh ab). The kernels keep no A/B knobs: what is left to pass are the probe macros
# (-DGNSS_CORR_PROBE=n for track.hip; SRC=vt -DGNSS_VT_PROBE=n for vt.hip; PROBE=1 adds the host's
# hooks) and compiler options. An experiment's own variant is a source change on a branch,
# built with tools/build_commit_lib.sh. Never used by the product, the tests or bench.py.
set -e
cd "$(dirname "$0")/../assignment-for-aae6102_gnss-sdr_amd/csrc"
make -s
mkdir -p ../../tools/probe_lib /tmp/gnss_variant_obj
NAME=$1; shift
SRC=${SRC:-track}
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -pthread -Wall -Wno-unused-function "$@" \
  -c $SRC.hip -o /tmp/gnss_variant_obj/${SRC}_$NAME.o
OBJS=$(make -s print-objs | tr ' ' '\n' | grep -v "/$SRC.o$")
if [ -n "$PROBE" ]; then  # PROBE=1: the host side's probe hooks too (GNSS_STAMPS, GNSS_PROBE environment)
  for h in $(grep -l "probe_env(" *.cpp | sed "s/\.cpp$//"); do  # the host files that call probe_env
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -pthread -DGNSS_PROBE_BUILD=1 \
      -c $h.cpp -o /tmp/gnss_variant_obj/${h}_$NAME.o
    OBJS="$(echo $OBJS | tr ' ' '\n' | grep -v "/${h}_host.o$" | tr '\n' ' ') /tmp/gnss_variant_obj/${h}_$NAME.o"
  done
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/probe_lib/libgnss_$NAME.so \
  /tmp/gnss_variant_obj/${SRC}_$NAME.o $OBJS -L/opt/rocm/lib -lrocfft -pthread -Wl,-rpath,/opt/rocm/lib
echo "built tools/probe_lib/libgnss_$NAME.so"
