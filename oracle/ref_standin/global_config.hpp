/*
 * global_config.hpp -- stand-in (TEST INFRASTRUCTURE ONLY, this project's own text).
 *
 * The reference's include/global_config.hpp pulls in Arduino.h and the debug / logger tasks.
 * The files oracle/Makefile compiles against this stand-in (VD_vehicle_controller.cpp,
 * VD_motor_if_m2006.cpp, imu_if_wt901c.cpp and the utility headers they include) use nothing
 * of it but the fixed-width integer types.
 */
#ifndef GLOBAL_CONFIG_HPP_
#define GLOBAL_CONFIG_HPP_

#include <stdint.h>

#endif
