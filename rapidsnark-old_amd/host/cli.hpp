// What the command-line programs share around their run(): the device from the environment, and the shell of main().
#pragma once
#include <cstdint>
#include <cstdlib>
#include <exception>
#include <iostream>

// ZKHIP_DEVICE=<n>, or -1: the current device
inline int32_t device_from_env() {
    const char *dev = getenv("ZKHIP_DEVICE");
    return dev ? atoi(dev) : -1;
}

// main(): the usage on a wrong number of arguments, else body()'s exit code; an exception's text goes to stderr.  Both
// failures leave with -1 (exit code 255), as the reference's `prover` does.
template <class Body>
int cli_main(bool argcOk, const char *usage, Body body) {
    if (!argcOk) {
        std::cerr << "Invalid number of parameters:\n";
        std::cerr << "Usage: " << usage << "\n";
        return -1;
    }
    try {
        return body();
    } catch (std::exception &e) {
        std::cerr << e.what() << '\n';
        return -1;
    }
}
