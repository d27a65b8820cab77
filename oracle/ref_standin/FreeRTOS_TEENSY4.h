/*
 * FreeRTOS_TEENSY4.h -- stand-in (TEST INFRASTRUCTURE ONLY, this project's own text; nothing
 * here is taken from FreeRTOS, the Teensy core or Arduino).
 *
 * What the reference's imu_if_wt901c.cpp needs besides the WT901 SDK: a HardwareSerial with
 * begin / write / flush / clear / available / read, the Serial6 object, vTaskDelay and the
 * general-purpose timer count it reads for its receive timeout.  The serial port is a byte
 * queue that oracle/ref_imu_harness.cpp fills; the definitions live there.
 */
#ifndef FREERTOS_TEENSY4_STANDIN_H_
#define FREERTOS_TEENSY4_STANDIN_H_

#include <stddef.h>
#include <stdint.h>

class HardwareSerial {
public:
  void   begin(uint32_t baud);
  size_t write(const uint8_t *data, size_t len);
  void   flush();
  void   clear();
  int    available();
  int    read();
};

extern HardwareSerial Serial6;

void vTaskDelay(uint32_t ticks);

extern "C" uint32_t get_gptimer_cnt();

#endif
