// The whole LocalMapping::CreateNewMapPoints of INTEGRATION.md over stand-in key frames, once, on the device: the program of
// newpts_shim_test.cpp with the library call in place of the injected outputs (tests/test_gpu_newpts.py compares the object
// graph it prints with the model's).
#define NEWPTS_RUN_ON_DEVICE 1
#include "newpts_shim_test.cpp"
