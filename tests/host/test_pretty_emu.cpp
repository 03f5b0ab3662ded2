// tests/host/test_pretty_emu.cpp -- CPU tier: the driver of tests/host/test_json_emu.cpp -- its records, its guards, its decisions -- around the PRETTY instantiations of
// the kernels of sjgpu_json.hip: the launch sequence of sjgpu_prettify_cells_device (include/sjgpu_pretty.h).  The two launchers are renamed in front of every header,
// so nothing below can reach the minify ones; a program of its own.  tests/test_pretty_emu.py compares what comes out with tests/pretty_model.py.
#define launch_json_count launch_pretty_count
#define launch_json_fill launch_pretty_fill
#include "sjgpu_pretty.h"
#include "test_json_emu.cpp"
