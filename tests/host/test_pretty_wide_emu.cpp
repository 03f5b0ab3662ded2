// tests/host/test_pretty_wide_emu.cpp -- CPU tier: the driver of tests/host/test_json_wide_emu.cpp -- its records, its guards, its decisions, SJGPU_E_RANGE among them --
// around the PRETTY instantiations of the kernels of sjgpu_json_wide.hip and the narrow count of sjgpu_json.hip: the launch sequence of
// sjgpu_prettify_cells_wide_device (include/sjgpu_pretty.h).  The three launchers are renamed in front of every header, so nothing below can reach the minify ones
// (launch_json_wide_extents is shared); a program of its own.  tests/test_pretty_wide_emu.py compares what comes out with tests/pretty_model.py.
#define launch_json_count launch_pretty_count
#define launch_json_wide_count launch_pretty_wide_count
#define launch_json_wide_fill launch_pretty_wide_fill
#include "sjgpu_pretty.h"
#include "test_json_wide_emu.cpp"
