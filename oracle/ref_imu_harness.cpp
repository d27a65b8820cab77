/*
 * ref_imu_harness.cpp -- driver around the REFERENCE's own IMT::IMU_IF_WT901C
 * (src/Imu/imu_if_wt901c.cpp with util_mymath.hpp, on top of the reference's WT901 SDK in
 * oracle/_ref/libwit_ref.so), compiled unmodified from /root/reference by oracle/Makefile into
 * oracle/_ref/libimu_ref.so.
 *
 * TEST INFRASTRUCTURE ONLY.  Three stand-in headers (oracle/ref_standin/) replace Arduino.h,
 * CMSIS-DSP and the RTOS: global_config.hpp (fixed-width integers), arm_math.h (PI; the trig
 * forwards are not used on this path) and FreeRTOS_TEENSY4.h, whose HardwareSerial is the byte
 * queue below.  The general-purpose timer stands still, so isComComp's receive timeout never
 * fires (why it does not on the firmware: fmskf_oracle.c, orc_wt901_is_com_comp).
 *
 * The SDK and the interface keep file-static state (sReg, s_cDataUpdate, the parser window),
 * so one process holds one scenario.  init() spins until a quaternion frame has arrived; on a
 * queue that runs dry first, the stand-in's available() ends the call with an error instead.
 */
#include <stdint.h>
#include <string.h>

#include "FreeRTOS_TEENSY4.h"
#include "imu_if_wt901c.hpp"

namespace {

const size_t QMAX = 1 << 16;
uint8_t g_q[QMAX];
size_t g_head, g_tail;
bool g_in_init, g_seen_empty;

struct QueueDry {};

IMT::IMU_IF_WT901C g_imu; /* static storage: zeroed before the constructor, like the firmware's */

void fill(const uint8_t *bytes, uint32_t len) {
  g_head = g_tail = 0;
  if (len > QMAX) len = QMAX;
  memcpy(g_q, bytes, len);
  g_tail = len;
}

}  // namespace

HardwareSerial Serial6;

void HardwareSerial::begin(uint32_t) {}
size_t HardwareSerial::write(const uint8_t *, size_t len) { return len; }
void HardwareSerial::flush() {}
void HardwareSerial::clear() { g_head = g_tail = 0; }
int HardwareSerial::available() {
  if (g_head == g_tail && g_in_init) {
    if (g_seen_empty) throw QueueDry(); /* init() would spin for ever: end the scenario */
    g_seen_empty = true;
  }
  return (int)(g_tail - g_head);
}
int HardwareSerial::read() { return g_head < g_tail ? g_q[g_head++] : -1; }

void vTaskDelay(uint32_t) {}

extern "C" uint32_t get_gptimer_cnt() { return 0; }

extern "C" {

/* IMU_IF_WT901C::init() with the bytes that answer its register read already queued.
 * Returns 0, or -1 when the bytes held no quaternion frame. */
int ref_imu_init(const uint8_t *bytes, uint32_t len) {
  fill(bytes, len);
  g_in_init = true;
  g_seen_empty = false;
  int rc = 0;
  try {
    g_imu.init();
  } catch (const QueueDry &) {
    rc = -1;
  }
  g_in_init = false;
  return rc;
}

/* one poll: the UART bytes that arrived since the last one, then update() */
void ref_imu_poll(const uint8_t *bytes, uint32_t len) {
  fill(bytes, len);
  g_imu.update();
}

/* isError() and getDataLatest(): accel[3] gyro[3] mag[3] angle[3] qut[4] */
int ref_imu_read(float data[16]) {
  IMT::IMU_IF::Data d;
  g_imu.getDataLatest(d);
  memcpy(data, &d, sizeof(float) * 16);
  return g_imu.isError() ? 1 : 0;
}

}  // extern "C"
